"""GPU: the resampler and the pose reductions at the particle counts where their code takes another path, held to exact
references.  One landmark per particle (a slot is 2 KB), so the sizes beyond 262 144 = kRedBlocks x 256 = kAncestorsScanMaxBlocks x
kScanBlock -- where k_summary_partials and k_block_max enter their grid-stride loops and pk_resample launches k_scan_blocks
instead of letting k_ancestors scan the block totals -- cost half a gigabyte and a fraction of a second; at the other end P = 1,
2, 3 and the straddles of a wave, a 256-lane workgroup and a 1 024-particle scan block.

Ancestors: tests/resample_reference.py::ancestors_match_exact (longdouble, from the downloaded log-weights; a derived
window, at most two slots).  Sums: math.fsum."""
import math

import numpy as np
import pytest

from oracle.fastslam_oracle import low_variance_ancestors_sequential, synthetic_world
from figures_record import record
from resample_reference import ancestors_match_exact

gpu = pytest.mark.gpu  # (every test but the first needs the card)

# (decades of weight spread, u) of tests/test_gpu_config2.py::test_ancestors_exact_at_scale_on_random_weights, seeded RandomState(P);
# the last with 70 % of the particles dead
RECIPES = [(0.0, 0.5), (3.0, 0.123456789), (12.0, 0.999), (200.0, 1e-9), (40.0, 0.31)]
U_EDGES = (0.0, 0.5, 1.0 - 2.0 ** -53)


def make_filter(lib, P):
    means, covs = synthetic_world(1)
    f = lib.DeviceFilter(P, 1)
    f.upload_map(means, covs.reshape(1, 25))
    return f


def base_poses(P):
    poses = np.zeros((P, 4))
    poses[:, 0] = np.arange(P)  # x says which particle a slot was gathered from
    poses[:, 1] = -0.5 * np.arange(P)
    poses[:, 2] = np.linspace(-3.0, 3.0, P)
    return poses


def recipe_weights(P):
    """The five weight vectors of RECIPES at P, drawn as the at-scale test draws them."""
    rs = np.random.RandomState(P)
    out = []
    for trial, (decades, u) in enumerate(RECIPES):
        w = 10.0 ** (-decades * rs.uniform(0, 1, P))
        if trial == 4:
            w[rs.uniform(0, 1, P) < 0.7] = 0.0
        out.append((w, u))
    return out


def resample_and_check(lib, f, poses, u, exact_expected=None):
    """Both weight domains: the ancestors against the exact resampler, the gathered poses and log-weights bit for bit.
    Returns the number of slots that differed from the exact resampler (inside its window)."""
    differing = 0
    for domain in (lib.PK_WEIGHTS_LINEAR, lib.PK_WEIGHTS_LOG):
        f.upload_poses(poses)  # (a resample gathers the poses: restore the generation)
        logw = f.download_log_weights()
        anc = f.resample(u, domain=domain, return_ancestors=True)
        if exact_expected is not None:
            assert np.array_equal(anc, exact_expected), (domain, u)
        differing += ancestors_match_exact(anc, logw, u, domain == lib.PK_WEIGHTS_LOG)
        got = f.download_poses()
        assert np.array_equal(got[:, :3], poses[anc, :3]), (domain, u)
        assert np.array_equal(f.download_log_weights(), logw[anc]), (domain, u)
    return differing


def test_equal_weights_at_u_zero_follow_the_reference_walk_on_the_host():
    """What case 1 asserts exactly, checked against the literal loop of prkt_core_v2.py:216-250 first: comb point k against
    C_j = j + 1 with '<=' (:239)."""
    assert np.array_equal(low_variance_ancestors_sequential(np.ones(5), 0.0), [0, 0, 1, 2, 3])


@gpu
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_small_and_straddling_particle_counts(lib, P):
    f = make_filter(lib, P)
    rs = np.random.RandomState(1000 + P)
    weights = [("random", rs.uniform(0.0, 1.0, P) ** 4), ("equal", np.ones(P))]
    for name, s in [("first", 0), ("last", P - 1), ("at 1023", 1023), ("at 1024", 1024)]:
        if s < P:
            w = np.zeros(P)
            w[s] = 1.0
            weights.append((name, w))
    for name, w in weights:
        poses = base_poses(P)
        poses[:, 3] = w
        for u in U_EDGES:
            # all weights 1.0 and u = 0 are exact in binary: the '<=' of the reference decides, no rounding does
            exact = np.maximum(np.arange(P) - 1, 0) if (name == "equal" and u == 0.0) else None
            resample_and_check(lib, f, poses, u, exact)
    f.close()


@gpu
@pytest.mark.parametrize("P", [262144, 262145, 300007])
def test_around_the_fused_scan_limit(lib, P):
    """262 144: 256 scan blocks, the last size k_ancestors scans itself; 262 145: 257, the first k_scan_blocks launch and the
    first grid-stride iteration of k_block_max."""
    f = make_filter(lib, P)
    assert f.shard_num_blocks() == (P + 1023) // 1024
    differing = 0
    for w, u in recipe_weights(P):
        poses = base_poses(P)
        poses[:, 3] = w
        differing += resample_and_check(lib, f, poses, u)
    f.close()
    print("P = %d: %d slots of %d resamples differ from the exact resampler" % (P, differing, 2 * len(RECIPES)))
    record("particle_edges", "resample_%d" % P, resamples=2 * len(RECIPES), slots_differing_from_the_exact_resampler=differing)


@gpu
def test_second_chunk_of_the_block_total_scan(lib):
    """2 050 scan blocks (2 049 full ones and one particle): k_scan_blocks goes round its 2 048-total chunk loop twice.  Two map
    buffers of 4.3 GB."""
    P = 2098177
    try:
        f = make_filter(lib, P)
    except lib.PkError as e:
        if e.status == lib.PK_ERR_NOMEM:
            pytest.skip("the card has no room for %d particles: %s" % (P, e))
        raise
    try:
        assert f.shard_num_blocks() == (P + 1023) // 1024 == 2050  # (beyond the 2 048 totals of one chunk)
        rs = np.random.RandomState(P)
        decades, u = RECIPES[1]
        poses = base_poses(P)
        poses[:, 3] = 10.0 ** (-decades * rs.uniform(0, 1, P))
        f.upload_poses(poses)
        logw = f.download_log_weights()
        anc = f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
        got = f.download_poses()
    finally:
        f.close()  # (before anything else is created)
    differing = ancestors_match_exact(anc, logw, u, True)
    assert np.array_equal(got[:, :3], poses[anc, :3])
    print("P = %d: %d slots differ from the exact resampler" % (P, differing))
    record("particle_edges", "resample_%d" % P, resamples=1, slots_differing_from_the_exact_resampler=differing)


def exact_sum(values):
    """The sum of a longdouble array to float64, exactly: every term split into two doubles for math.fsum."""
    v = np.asarray(values, dtype=np.longdouble)
    hi = v.astype(np.float64)
    lo = (v - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


@gpu
@pytest.mark.parametrize("P", [1, 255, 257, 262144, 262145, 300007])
def test_pose_sums_summary_and_maximum_weight(lib, P):
    """Tolerance 64 eps sum|term| per sum: a thread's chain is at most ceil(P / 262 144) additions, the workgroup's tree adds
    6 + 3, the final kernel at most 4 + 6 + 3, the library's sincos is below 1 ulp per term -- 64 covers it with a factor two to
    spare."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy.longdouble is no wider than float64 here: no reference for sin / cos")
    eps = np.finfo(np.float64).eps
    f = make_filter(lib, P)
    seed = 77 + P
    while True:
        rs = np.random.RandomState(seed)
        poses = np.ones((P, 4))
        poses[:, 0] = rs.uniform(-1e3, 1e3, P)
        poses[:, 1] = rs.uniform(-1e3, 1e3, P)
        poses[:, 2] = rs.uniform(-math.pi, math.pi, P)
        hl = poses[:, 2].astype(np.longdouble)
        sl, cl = np.sin(hl), np.cos(hl)
        ref = [math.fsum(poses[:, 0]), math.fsum(poses[:, 1]), exact_sum(sl), exact_sum(cl)]
        if abs(ref[2]) + abs(ref[3]) >= 1e-6 * P:
            break
        seed += 1000  # the mean heading of this draw is ill-conditioned: another draw, not an excuse
    mags = [math.fsum(np.abs(poses[:, 0])), math.fsum(np.abs(poses[:, 1])), exact_sum(np.abs(sl)), exact_sum(np.abs(cl))]
    # one weight zero, the largest at the very end: the maximum a grid-stride loop must not miss
    w = rs.uniform(0.1, 1.0, P)
    if P > 1:
        w[P // 3] = 0.0
    w[P - 1] = 2.0
    poses[:, 3] = w
    f.upload_poses(poses)
    sums = f.pose_sums()
    for i, name in enumerate(("x", "y", "sin", "cos")):
        err = abs(sums[i] - ref[i])
        print("P = %d sum %s: error %.3g, %.3g of the tolerance" % (P, name, err, err / (64 * eps * mags[i])))
        assert err <= 64 * eps * mags[i], (name, sums[i], ref[i])
    x, y, heading = f.summary()
    assert x == sums[0] / P and y == sums[1] / P
    want = float(np.arctan2(np.longdouble(ref[2]), np.longdouble(ref[3])))
    ulps = abs(heading - want) / np.spacing(abs(want))
    print("P = %d heading: %.3g ulp" % (P, ulps))
    record("particle_edges", "pose_sums_%d" % P, summary_heading_ulp=float(ulps),
           worst_fraction_of_64_eps_tolerance=max(abs(sums[i] - ref[i]) / (64 * eps * mags[i]) for i in range(4)))
    assert ulps <= 4.0, (heading, want)
    logw = f.download_log_weights()
    assert np.isneginf(logw).sum() == (1 if P > 1 else 0) and np.argmax(logw) == P - 1
    assert f.shard_max_logw() == logw.max()
    f.close()


@gpu
@pytest.mark.parametrize("P", [1025, 262145])
def test_every_weight_zero_in_the_log_domain(lib, P):
    f = make_filter(lib, P)
    poses = base_poses(P)  # weights 0: log-weights all -inf
    f.upload_poses(poses)
    assert np.isneginf(f.download_log_weights()).all()
    anc = f.resample(0.37, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True)
    assert np.all(anc == 0)
    got = f.download_poses()
    assert not np.isnan(got).any()
    assert np.array_equal(got[:, :3], poses[anc, :3])
    f.close()

"""GPU: unique data association (pk_assoc_unique, k_assoc_unique; DESIGN.md section 4, "Unique association") against
tests/assoc_unique_reference.py -- the shapes that cross the wave, the workgroup and the per-lane landmark loop, a displacement
chain, exact ties, all three function sets behind both association kernels, maps read through src[], growing maps, pk_associate
and the steps, the refusals, and the mode off left what it was.

ids, counters and potential flags exactly; means, covariances and log-weights to the tolerances of tests/test_gpu_bearing_model.py
(RTOL = 1e-9).  Before every comparison the oracle's own state is held to: no bearing gate within 1e-9 of turning, no colour gate
within 1e-6, and -- in every particle with a conflict -- no two positive probabilities of one blob or of one landmark within a
relative 1e-9 of each other, and none below 1e-300 (in the normal range: the device must not see it underflow).  A scene that violates one fails.
The exact-tie scene is built from bit-identical rows and is exempt from the gap: it tests the tie order."""
import math

import numpy as np
import pytest

import bearing_model_reference as ref
import grow_init_reference as gi
from assoc_unique_reference import uniquely
from bearing_model_reference import BearingOracle, under_bearing_model, wrapped_scan
from conftest import relerr
from oracle.fastslam_oracle import (EMPTY_COLOUR, GrowingOracle, OracleFilter, low_variance_ancestors, synthetic_scan,
                                    synthetic_world, truth_step)
from range_bearing_reference import RangeBearingOracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
GAP = 1e-9
FLOOR = 1e-300  # clear of the denormals (below 2.2e-308), where a probability no longer has its relative precision
ORACLES = {"reference": OracleFilter, "bearing": BearingOracle, "range": RangeBearingOracle}


# ---------------------------------------------------------------------------------------------------------------- helpers
def _assert_margins(o, blobs, what, bearing=True):
    """No gate of any (particle, landmark, blob) of the oracle's current state can be turned by rounding."""
    sx, sy, sh = o.x[:, None], o.y[:, None], o.h[:, None]
    for b in range(len(blobs)):
        if bearing:
            mb, mc = ref.gate_margins(sx, sy, sh, blobs[b], o.mean)
        else:  # the reference model: the difference as it comes, and the half-plane test of :473-475 beside the gates
            pse = np.arctan2(o.mean[..., 1] - sy, o.mean[..., 0] - sx)
            mb = np.minimum(np.abs(np.abs(blobs[b][0] - (pse - sh)) - 0.5), np.abs(np.abs(pse - blobs[b][0]) - math.pi / 2))
            mc = ref.gate_margins(sx, sy, sh, blobs[b], o.mean)[1]
        assert mb.min() > 1e-9 and mc.min() > 1e-6, (what, b, mb.min(), mc.min())


def _assert_decisive(o, what, ties=False):
    assert ties or o.unique_gap >= GAP, (what, o.unique_gap)
    assert o.unique_floor > FLOOR, (what, o.unique_floor)


def _cluster_world(L, seed):
    """L landmarks in the front sector whose colours come in clusters of about eight: a blob that loses its landmark has others."""
    rs = np.random.RandomState(seed)
    phi, rho = rs.uniform(-1.3, 1.3, L), rs.uniform(8.0, 30.0, L)
    centres = rs.uniform(30.0, 225.0, (max(1, L // 8), 3))
    means = np.empty((L, 5))
    means[:, 0], means[:, 1] = rho * np.cos(phi), rho * np.sin(phi)
    means[:, 2:] = centres[rs.randint(len(centres), size=L)] + rs.uniform(-5.0, 5.0, (L, 3))
    covs = np.broadcast_to(np.diag([1.0, 1.0, 4.0, 4.0, 4.0]), (L, 5, 5)).copy()
    return means, covs, rs


def _conflict_scan(means, B, rs, ranged=False):
    """B blobs that show landmarks of the first half of the map, several of them the same one: (blobs, ranges, variances)."""
    j = rs.randint(0, max(1, len(means) // 2), B)
    blobs = np.empty((B, 4))
    blobs[:, 0] = np.arctan2(means[j, 1], means[j, 0]) + 0.02 * rs.standard_normal(B)
    blobs[:, 1:] = means[j, 2:] + rs.standard_normal((B, 3))
    if not ranged:
        return blobs, None, None
    rho = np.hypot(means[j, 0], means[j, 1]) + 0.2 * rs.standard_normal(B)
    rho[1::3] = np.nan  # every third blob has no range
    return blobs, rho, np.full(B, 0.04)


def _poses(P, rs):
    xyhw = np.zeros((P, 4))
    xyhw[:, :2] = 0.3 * rs.standard_normal((P, 2))
    xyhw[:, 2] = 0.03 * rs.standard_normal(P)
    xyhw[:, 3] = 1.0
    return xyhw


def _pair(lib, model, P, means, covs, xyhw, opts=None, unique=True):
    L = len(means)
    f = lib.DeviceFilter(P, L)
    if model != "reference":
        f.set_measurement_model("bearing")
    for k, v in (opts or {}).items():
        f.set_option(k, v)
    f.upload_map(means, np.asarray(covs).reshape(L, 25))
    f.upload_poses(xyhw)
    o = ORACLES[model](P, means, covs)
    o.x[:], o.y[:], o.h[:] = xyhw[:, 0], xyhw[:, 1], xyhw[:, 2]
    if unique:
        f.assoc_unique(True)
        assert f.assoc_unique_state()
        uniquely(o)
    return f, o


def _compare_state(lib, f, o, what):
    got = f.download_log_weights()
    assert np.allclose(got, o.logw, rtol=0, atol=RTOL), (what, np.abs(got - o.logw).max())
    m, c, k = f.download_landmarks()
    assert np.array_equal((k & lib.PK_LANDMARK_POTENTIAL) != 0, o.potential), what
    assert np.array_equal(k & ~lib.PK_LANDMARK_POTENTIAL, o.count), what
    assert relerr(m, o.mean) < RTOL, (what, relerr(m, o.mean))
    assert np.allclose(c.reshape(o.cov.shape), o.cov, rtol=RTOL, atol=1e-13), what


def _observe_both(lib, f, o, blobs, rho, var, what, model, ties=False):
    """One fresh observe of the scan on the oracle and the device; ids, counters and state compared.  Returns the ids."""
    kw = dict(ranges=rho, variances=var) if rho is not None else {}
    _assert_margins(o, blobs, what, bearing=model != "reference")
    o.reset_weights()
    want = o.observe(blobs, **kw)
    _assert_decisive(o, what, ties)
    if rho is not None:
        f.scan_ranges(rho, var)
    got = f.observe(blobs, return_ids=True, fresh=True)
    assert f.observe_route() == "ml_general", what
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:5])
    assert tuple(f.assoc_unique_stats()) == o.unique_stats, (what, f.assoc_unique_stats(), o.unique_stats)
    _compare_state(lib, f, o, what)
    return want


# ---------------------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("B,L,P", [(1, 3, 1), (2, 3, 70), (63, 65, 70), (64, 300, 1), (65, 65, 70), (257, 300, 70), (300, 600, 70),
                                   (257, 600, 1)])
def test_shapes_across_the_wave_the_workgroup_and_the_landmark_loop(lib, B, L, P):
    means, covs, rs = _cluster_world(L, 1000 + 7 * B + L)
    f, o = _pair(lib, "bearing", P, means, covs, _poses(P, rs))
    blobs, _, _ = _conflict_scan(means, B, rs)
    ids = _observe_both(lib, f, o, blobs, None, None, (B, L, P), "bearing")
    for i in range(P):
        taken = ids[i][ids[i] > 0]
        assert len(np.unique(taken)) == len(taken)
    if B >= 2:
        assert o.unique_stats[0] >= 1 and o.unique_stats[1] >= 1  # the scene has conflicts
    if B >= 63:
        assert o.unique_stats[2] >= 1 and o.unique_stats[3] >= 3  # ... blobs that moved on to another landmark, in several passes
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 2. chain, ties
def _line_map(ys, colour=(120.0, 80.0, 60.0)):
    means = np.array([[10.0, y, *colour] for y in ys])
    return means, np.broadcast_to(np.identity(5), (len(ys), 5, 5)).copy()


def test_a_displacement_chain_and_a_blob_that_exhausts_its_list(lib):
    """Landmarks on the line x = 10 at y = 0, 1, 2.6, all of one colour; the rays of four blobs cross it at 0.05, 1.75, 0.4, 3.6.
    Blob 2 loses landmark 1 to blob 0; its second choice displaces blob 1 from landmark 2, whose second choice displaces blob 3 from
    landmark 3, and blob 3 can win nowhere else: four passes, ids 1 3 2 0."""
    means, covs = _line_map([0.0, 1.0, 2.6])
    P = 3
    xyhw = np.zeros((P, 4))
    xyhw[:, 3] = 1.0
    f, o = _pair(lib, "bearing", P, means, covs, xyhw)
    t = np.array([0.05, 1.75, 0.4, 3.6])
    blobs = np.empty((4, 4))
    blobs[:, 0] = np.arctan2(t, 10.0)
    blobs[:, 1:] = means[0, 2:] + np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 0.3], [0.2, 0.1, 0.0]])
    ml = BearingOracle.associate(o, blobs)
    ids = _observe_both(lib, f, o, blobs, None, None, "chain", "bearing")
    assert (ml == [1, 2, 1, 3]).all() and (ids == [1, 3, 2, 0]).all()
    stats = f.assoc_unique_stats()
    assert stats[3] == 4 and stats[0] == P and stats[1] == 3 * P and stats[2] == 2 * P
    f.close()


def test_exact_ties_go_to_the_lower_blob_then_the_lower_landmark(lib):
    """Bit-identical inputs: blobs 0 and 1 are one blob twice, landmarks 2 and 3 are one landmark twice (equal rows give equal bits
    on any arithmetic).  Blob 0 keeps the lower landmark, blob 1 takes the higher; a third identical blob ends 0."""
    means, covs = _line_map([-4.0, 1.0, 1.0, 6.0])
    means[[0, 3], 2] += 100.0  # (the outer two fail the colour gate)
    P = 2
    xyhw = np.zeros((P, 4))
    xyhw[:, 3] = 1.0
    for kernel in (0, 1):
        f, o = _pair(lib, "bearing", P, means, covs, xyhw, opts={"assoc_kernel": kernel})
        one = [math.atan2(1.2, 10.0), 121.0, 80.5, 60.0]
        blobs = np.array([one, one, one])
        ids = _observe_both(lib, f, o, blobs, None, None, ("ties", kernel), "bearing", ties=True)
        assert (ids == [2, 3, 0]).all()
        f.close()


# ---------------------------------------------------------------------------------------------------------------- 3. function sets
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("model", ["reference", "bearing", "range"])
def test_all_three_function_sets_behind_both_association_kernels(lib, model, kernel):
    L, B, P = 48, 60, 32
    means, covs, rs = _cluster_world(L, 77)
    f, o = _pair(lib, model, P, means, covs, _poses(P, rs), opts={"assoc_kernel": kernel})
    blobs, rho, var = _conflict_scan(means, B, rs, ranged=model == "range")
    _observe_both(lib, f, o, blobs, rho, var, (model, kernel), model)
    assert o.unique_stats[0] == P and o.unique_stats[2] >= 1
    if model == "range":
        assert np.isnan(rho).any() and not np.isnan(rho).all()
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 4. src[], uploads
def test_maps_read_through_the_resample_and_single_particle_uploads(lib):
    """Three scans: the second comes behind a resample with no observe in between -- the kernel reads every map through src[] --, the
    third behind pk_upload_landmarks on single particles, whose conflicts then differ from their neighbours'."""
    L, B, P = 40, 44, 32
    means, covs, rs = _cluster_world(L, 31)
    f, o = _pair(lib, "bearing", P, means, covs, _poses(P, rs))
    # (a colour noise that keeps the colour blocks from collapsing within two updates: the losers' far candidates stay in the normal range)
    o.Qt = np.diag([0.05, 4.0, 4.0, 4.0])
    f.set_measurement_noise(o.Qt)
    per_particle = []
    for s in range(3):
        if s == 2:
            for i in (3, 17):
                m, c, k = f.download_landmarks(i, i + 1)
                m[0, :L // 2, :2] += rs.uniform(-1.5, 1.5, (L // 2, 2))
                f.upload_landmarks(i, i + 1, means=m, covs=c, counts=k)
                o.mean[i] = m[0]
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        blobs, _, _ = _conflict_scan(means, B, rs)
        o.motion(0.4, 0.05, 0.5, z)
        f.motion(0.4, 0.05, 0.5, z=z)
        ids = _observe_both(lib, f, o, blobs, None, None, ("scan", s), "bearing")
        per_particle.append(ids)
        anc = low_variance_ancestors(np.exp(o.logw - np.max(o.logw)), u)
        assert np.array_equal(f.resample(u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), anc), s
        o.gather(anc)
        if s == 0:
            assert len(np.unique(anc)) < P  # the next scan's maps are read through src[]
    assert any((per_particle[2][i] != per_particle[2][0]).any() for i in (3, 17))
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 5. conflict-free
@pytest.mark.parametrize("model", ["reference", "bearing"])
def test_a_conflict_free_drive_is_the_drive_of_a_filter_that_never_asked(lib, model):
    L, P = 40, 128
    means, covs = synthetic_world(L)
    xyhw = np.zeros((P, 4))
    xyhw[:, 3] = 1.0
    fa, _ = _pair(lib, model, P, means, covs, xyhw, unique=False)
    fb, _ = _pair(lib, model, P, means, covs, xyhw, unique=False)
    fb.assoc_unique(True)
    rs = np.random.RandomState(4)
    pose = (0.0, 0.0, 0.0)
    for s in range(4):
        pose = truth_step(pose, 0.2, 0.1, 0.5)
        blobs = synthetic_scan(means, pose) if model == "reference" else wrapped_scan(means, pose)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        ids = []
        for f in (fa, fb):
            f.motion(0.2, 0.1, 0.5, z=z)
            ids.append(f.observe(blobs, return_ids=True, fresh=True))
        assert np.array_equal(ids[0], ids[1]), s
        for i in range(P):
            taken = ids[0][i][ids[0][i] > 0]
            assert len(np.unique(taken)) == len(taken), "the scene is not conflict-free"
        assert tuple(fb.assoc_unique_stats()) == (0, 0, 0, 1) and tuple(fa.assoc_unique_stats()) == (0, 0, 0, 0)
        assert np.array_equal(fa.download_log_weights(), fb.download_log_weights()), s
        for a, b in zip(fa.download_landmarks(), fb.download_landmarks()):
            assert np.array_equal(a, b), s
        assert np.array_equal(fa.resample(u, return_ancestors=True), fb.resample(u, return_ancestors=True)), s
        assert np.array_equal(fa.download_poses(), fb.download_poses()), s
    fa.close()
    fb.close()


# ---------------------------------------------------------------------------------------------------------------- 6. growing maps
C = gi.SMALL


def _twin_world():
    """The small scene's world with a fourteenth landmark: the twin of preset landmark 1 -- its colour, 2 m beside it."""
    world, covs = gi.small_world()
    twin = world[0].copy()
    r = math.hypot(world[0, 0], world[0, 1])
    twin[0] += -2.0 * world[0, 1] / r  # (across the line of sight from the origin)
    twin[1] += 2.0 * world[0, 0] / r
    return np.vstack([world, twin]), covs


@pytest.mark.parametrize("name", ["reference_rule", "bearing_0.1", "bearing_0.1_retiring"])
def test_growing_maps_step_by_step_on_the_small_scene_with_a_twin(lib, name):
    """The small scene of test_gpu_grow.py / test_gpu_grow_init.py under the bearing model, to which a twin of a preset landmark is
    added: both rules of landmark_init, one case with retirement.  Counters, readings, slot ids, clocks, maps and log-weights against
    the growing oracle with the mixin at every step; the twin is found in every particle."""
    world, covs = _twin_world()
    L0, retire = C["L0"], None
    means, mcov = gi.small_map()
    f = lib.DeviceFilter(C["P"], len(means))
    f.set_measurement_model("bearing")
    f.upload_map(means, mcov.reshape(len(means), 25))
    if name == "reference_rule":
        f.grow_enable(L0, 64, C["thr"])
        o = under_bearing_model(GrowingOracle(C["P"], world[:L0], covs[:L0], C["spare"], C["thr"]))
        seed = 6
    else:
        _model, mp, R, retire, seed = gi.GPU_SCENES[name]
        f.grow_enable(L0, R, C["thr"])
        if retire:
            f.grow_retire(*retire)
        f.grow_init("triangulated", mp)
        o = gi.small_oracle(name)
    uniquely(o)
    f.assoc_unique(True)
    conflicts = 0
    for st in gi.drive(o, world, C["steps"], seed, C["v"], C["w"], C["dt"], gi.noise_free_wrapped):
        assert st.gates[0] > 1e-9 and st.gates[1] > 1e-6, (st.s, st.gates)
        _assert_decisive(o.f, st.s)
        f.motion(C["v"], C["w"], C["dt"], z=st.z)
        f.observe(st.blobs, fresh=True)
        assert f.observe_route() == "ml_general"
        assert tuple(f.assoc_unique_stats()) == o.f.unique_stats, (st.s, f.assoc_unique_stats(), o.f.unique_stats)
        conflicts += o.f.unique_stats[0]
        got = f.download_log_weights()
        assert np.allclose(got, st.logw, rtol=0, atol=RTOL), (st.s, np.abs(got - st.logw).max())
        assert np.array_equal(f.resample(st.u, domain=lib.PK_WEIGHTS_LOG, return_ancestors=True), st.anc), st.s
        st.finish()
        cnt, rd, sid = f.grow_download()
        assert np.array_equal(cnt[:, 0], [len(h) for h in o.hyp]) and np.array_equal(cnt[:, 1], o.used), st.s
        assert np.array_equal(cnt[:, 2], o.next_id) and not cnt[:, 3].any(), st.s
        for i in range(f.P):
            n, used = int(cnt[i, 0]), int(cnt[i, 1])
            if n:
                assert np.allclose(rd[i, :n], np.asarray(o.hyp[i]), rtol=1e-12, atol=1e-12), (st.s, i)
            assert [int(v) for v in sid[i, :used]] == [o.slot_id[i][L0 + k] for k in range(used)], (st.s, i)
        if retire:
            kc, _sc, _se, _si, now = f.grow_clocks_download()
            assert now == o.t and np.array_equal(kc, o.clock_counters()), st.s
        m, c, k = f.download_landmarks()
        assert np.array_equal((k & lib.PK_LANDMARK_POTENTIAL) != 0, o.f.potential), st.s
        assert np.array_equal(k & ~lib.PK_LANDMARK_POTENTIAL, o.f.count), st.s
        assert relerr(m, o.f.mean) < RTOL, (st.s, relerr(m, o.f.mean))
        assert np.allclose(c.reshape(o.f.cov.shape), o.f.cov, rtol=RTOL, atol=1e-13), st.s
    assert conflicts >= C["P"]                   # the twin's blob and its landmark's claimed one landmark
    # the three unknown landmarks of the scene AND the twin, in every particle (with readings retired after four scans: in some)
    assert max(o.used) >= 4 and min(o.used) >= (3 if retire else 4)
    assert (o.f.count[:, 0] <= 2 * C["steps"]).all()  # the preset twin: one update a scan at most (two counts each)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 7. associate, steps
def _conflict_filter(lib, seed=5, P=32):
    L, B = 40, 48
    means, covs, rs = _cluster_world(L, seed)
    xyhw = _poses(P, rs)
    blobs, _, _ = _conflict_scan(means, B, rs)
    return means, covs, xyhw, blobs, rs


def _downloads(f):
    return [f.download_poses(), f.download_log_weights(), *f.download_landmarks()]


def test_associate_returns_the_settled_ids_and_changes_nothing(lib):
    means, covs, xyhw, blobs, rs = _conflict_filter(lib)
    P = len(xyhw)
    f, o = _pair(lib, "bearing", P, means, covs, xyhw)
    before = _downloads(f)
    _assert_margins(o, blobs, "associate")
    want = o.associate(blobs)
    _assert_decisive(o, "associate")
    assert np.array_equal(f.associate(blobs), want)
    assert tuple(f.assoc_unique_stats()) == o.unique_stats and o.unique_stats[0] == P
    assert (BearingOracle.associate(o, blobs) != want).any()
    for a, b in zip(before, _downloads(f)):
        assert np.array_equal(a, b)
    f.close()


@pytest.mark.parametrize("step", ["step", "step_adaptive", "step_odom"])
def test_the_steps_take_the_mode(lib, step):
    """pk_step, pk_step_adaptive and pk_step_odom against the same calls made one by one, bit for bit, on a scan with conflicts."""
    means, covs, xyhw, blobs, rs = _conflict_filter(lib, seed=9)
    P = len(xyhw)
    fa, _ = _pair(lib, "bearing", P, means, covs, xyhw)
    fb, _ = _pair(lib, "bearing", P, means, covs, xyhw)
    z, u = rs.standard_normal((P, 3)), 0.37
    delta, alphas = (0.02, 0.3, 0.01), (0.05, 0.01, 0.05, 0.01)
    if step == "step":
        fa.motion(0.4, 0.05, 0.5, z=z)
        fa.observe(blobs, fresh=True)
        fa.resample(u)
        fb.step(0.4, 0.05, 0.5, blobs, u, z=z)
    elif step == "step_adaptive":
        fa.motion(0.4, 0.05, 0.5, z=z)
        fa.observe(blobs)
        fa.resample_adaptive(u, 2.0)
        fb.step_adaptive(0.4, 0.05, 0.5, blobs, u, 2.0, z=z)
    else:
        fa.motion_odom(delta, alphas, z=z)
        fa.observe(blobs, fresh=True)
        fa.resample(u)
        fb.step_odom(delta, alphas, blobs, u, z=z)
    sa, sb = fa.assoc_unique_stats(), fb.assoc_unique_stats()
    assert tuple(sa) == tuple(sb) and sb[0] == P and sb[1] > 0
    assert fb.observe_route() == "ml_general"
    for a, b in zip(_downloads(fa), _downloads(fb)):
        assert np.array_equal(a, b)
    fa.close()
    fb.close()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals, lifecycle
def _refused(lib, call, status=None):
    status = lib.PK_ERR_UNSUPPORTED if status is None else status
    with pytest.raises(lib.PkError) as e:
        call()
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_refusals_and_lifecycle(lib):
    means, covs, xyhw, blobs, rs = _conflict_filter(lib, seed=13)
    P, L = len(xyhw), len(means)
    f, o = _pair(lib, "bearing", P, means, covs, xyhw, unique=False)
    assert f.assoc_unique_state() is False and tuple(f.assoc_unique_stats()) == (0, 0, 0, 0)
    bytes0 = f.device_bytes()
    for bad in (2, -1):
        _refused(lib, lambda: lib.check(f._lib.pk_assoc_unique(f._h, bad)), lib.PK_ERR_INVALID)
    assert f.assoc_unique_state() is False and f.device_bytes() == bytes0
    # switching the mode between scans: the ids are the mode's of the moment
    ml = o.associate(blobs)
    assert np.array_equal(f.associate(blobs), ml)
    bytes1 = f.device_bytes()  # (the association's own buffers came with the first scan)
    f.assoc_unique(True)
    assert f.device_bytes() == bytes1 + 64
    uniquely(o)
    un = o.associate(blobs)
    _assert_decisive(o, "switch")
    assert np.array_equal(f.associate(blobs), un) and (un != ml).any()
    f.assoc_unique(False)
    assert np.array_equal(f.associate(blobs), ml) and tuple(f.assoc_unique_stats()) == (0, 0, 0, 0)
    f.assoc_unique(True)
    # the proposal and the split observe are refused, nothing changed
    before = _downloads(f)
    msg = _refused(lib, lambda: f.propose(0.4, 0.05, 0.5, blobs, z=np.zeros((P, 3))))
    assert "pk_assoc_unique" in msg and "k_propose" in msg
    _refused(lib, lambda: f.propose_odom((0.0, 0.3, 0.0), (0.05, 0.01, 0.05, 0.01), blobs, z=np.zeros((P, 3))))
    for a, b in zip(before, _downloads(f)):
        assert np.array_equal(a, b)
    f.set_measurement_model("reference")
    f.stage_scan(blobs)
    _refused(lib, lambda: f.observe_staged_range(True, 0, P, True, True))
    f.observe_staged(fresh=True)  # (the staged scan is still there, and takes the mode)
    assert f.observe_route() == "ml_general" and f.assoc_unique_stats()[0] > 0
    f.close()
    f, o = _pair(lib, "bearing", P, means, covs, xyhw)
    # supplied ids are applied as ever
    ids = np.zeros(len(blobs), dtype=np.int32)
    ids[:3] = [1, 1, 2]
    g, _ = _pair(lib, "bearing", P, means, covs, xyhw, unique=False)
    f.observe(blobs, ids=ids, fresh=True)
    g.observe(blobs, ids=ids, fresh=True)
    assert f.observe_route() == "known_ids" and tuple(f.assoc_unique_stats()) == (0, 0, 0, 0)
    for a, b in zip(_downloads(f), _downloads(g)):
        assert np.array_equal(a, b)
    f.close()
    g.close()


def test_the_dense_layout_and_a_scan_beyond_lds_are_refused(lib):
    L, P = 6, 4
    means, covs = synthetic_world(L)
    dense = covs.copy()
    dense[:, 0, 2] = dense[:, 2, 0] = 0.01  # position and colour coupled: the dense layout
    f = lib.DeviceFilter(P, L)
    f.upload_map(means, dense.reshape(L, 25))
    f.assoc_unique(True)
    blobs = synthetic_scan(means, (0.0, 0.0, 0.0))
    before = _downloads(f)
    assert "dense layout" in _refused(lib, lambda: f.observe(blobs, fresh=True))
    assert "dense layout" in _refused(lib, lambda: f.associate(blobs))
    for a, b in zip(before, _downloads(f)):
        assert np.array_equal(a, b)
    f.observe(blobs, ids=np.arange(1, L + 1, dtype=np.int32), fresh=True)  # supplied ids: as ever
    assert f.observe_route() == "dense"
    f.close()
    # 12 bytes per padded landmark + 14 per blob against the workgroup's LDS: refused before anything is launched
    L, B = 9000, 4000
    means, covs = synthetic_world(L)
    f = lib.DeviceFilter(1, L)
    f.upload_map(means, covs.reshape(L, 25))
    blobs = synthetic_scan(means, (0.0, 0.0, 0.0))[:B]
    f.assoc_unique(True)
    before = _downloads(f)
    msg = _refused(lib, lambda: f.observe(blobs, fresh=True))
    assert "12 x" in msg and "14 x %d" % B in msg
    assert "12 x" in _refused(lib, lambda: f.associate(blobs))
    for a, b in zip(before, _downloads(f)):
        assert np.array_equal(a, b)
    f.assoc_unique(False)
    f.observe(blobs, fresh=True)  # the same scan with the mode off
    f.synchronize()
    f.close()


# ---------------------------------------------------------------------------------------------------------------- 9. off is today
@pytest.mark.parametrize("model", ["reference", "bearing"])
def test_off_is_today(lib, model):
    """A filter on which the new calls were made with the mode off against one on which they never were: the launch counts of
    pk_timings per slot, pk_device_bytes and every download of a short drive."""
    L, P = 40, 256
    means, covs = synthetic_world(L)
    xyhw = np.zeros((P, 4))
    xyhw[:, 3] = 1.0
    fa, _ = _pair(lib, model, P, means, covs, xyhw, unique=False)
    fb, _ = _pair(lib, model, P, means, covs, xyhw, unique=False)
    fb.assoc_unique(False)
    assert fb.assoc_unique_state() is False and tuple(fb.assoc_unique_stats()) == (0, 0, 0, 0)
    assert fa.device_bytes() == fb.device_bytes()
    for f in (fa, fb):
        f.enable_timing(True)
    rs = np.random.RandomState(8)
    pose = (0.0, 0.0, 0.0)
    for s in range(3):
        pose = truth_step(pose, 0.2, 0.1, 0.5)
        world = np.vstack([means, means[:2]])  # two landmarks are seen twice: the maximum-likelihood ids claim them twice, as today
        blobs = synthetic_scan(world, pose) if model == "reference" else wrapped_scan(world, pose)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        for f in (fa, fb):
            f.motion(0.2, 0.1, 0.5, z=z)
            f.observe(blobs, fresh=True)
            f.associate(blobs)
            f.resample(u)
        assert fa.observe_route() == fb.observe_route()
        for a, b in zip(_downloads(fa), _downloads(fb)):
            assert np.array_equal(a, b), s
        fb.assoc_unique_stats()
    na, nb = {k: n for k, (_ms, n) in fa.timings().items()}, {k: n for k, (_ms, n) in fb.timings().items()}
    assert na == nb and sum(na.values()) > 0, (na, nb)
    assert fa.device_bytes() == fb.device_bytes()
    fa.close()
    fb.close()


# ---------------------------------------------------------------------------------------------------------------- 10. steps refused, split, facade
def test_a_step_refused_in_the_mode_moves_nothing(lib):
    """pk_step, pk_step_adaptive and pk_step_odom with the mode on: the dense layout and a scan beyond LDS are refused ahead of the
    motion -- the poses, the weights and the maps are what they were."""
    L, P = 6, 4
    means, covs = synthetic_world(L)
    dense = covs.copy()
    dense[:, 0, 2] = dense[:, 2, 0] = 0.01
    small = synthetic_scan(means, (0.0, 0.0, 0.0))
    big_means, big_covs = synthetic_world(9000)
    big = synthetic_scan(big_means, (0.0, 0.0, 0.0))[:4000]
    for m, c, blobs, word in ((means, dense, small, "dense layout"), (big_means, big_covs, big, "12 x")):
        n = len(m)
        f = lib.DeviceFilter(P if n == L else 1, n)
        f.upload_map(m, c.reshape(n, 25))
        f.assoc_unique(True)
        before = _downloads(f)
        z = np.ones((f.P, 3))
        assert word in _refused(lib, lambda: f.step(0.4, 0.05, 0.5, blobs, 0.3, z=z))
        assert word in _refused(lib, lambda: f.step(0.4, 0.05, 0.5, blobs, 0.3, seed=3, draw=1))  # (the launch that moves and uploads at once)
        assert word in _refused(lib, lambda: f.step_adaptive(0.4, 0.05, 0.5, blobs, 0.3, 2.0, z=z))
        assert word in _refused(lib, lambda: f.step_odom((0.02, 0.3, 0.01), (0.05, 0.01, 0.05, 0.01), blobs, 0.3, z=z))
        for a, b in zip(before, _downloads(f)):
            assert np.array_equal(a, b), word
        f.close()


def test_the_mode_cannot_be_switched_inside_a_split_observe(lib):
    L, P = 600, 64
    means, covs = synthetic_world(L)
    f = lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    f.stage_scan(synthetic_scan(means, (0.0, 0.0, 0.0)))
    assert f.staged_takes_regs()
    f.observe_staged_range(True, 0, P // 2, True, False)
    for on in (1, 0):
        _refused(lib, lambda: lib.check(f._lib.pk_assoc_unique(f._h, on)), lib.PK_ERR_STATE)
    assert f.assoc_unique_state() is False
    f.observe_staged_range(True, P // 2, P, False, True)
    f.assoc_unique(True)
    assert f.assoc_unique_state() is True
    f.close()


class _Scan(object):
    def __init__(self, blobs):
        self.last_sensor_reading = type("Reading", (), {})()
        self.last_sensor_reading.observes = blobs


def _facade_drive(association, steps=14):
    import random

    import parakeet_slam_amd as pk
    import assoc_unique_reference as uq

    d = uq.TWIN_DRIVE
    cov = 0.25 * np.identity(5)
    feats = [pk.Feature(mean=m.copy(), covar=cov.copy()) for m in uq.TWIN_KNOWN]
    np.random.seed(11)
    random.seed(7)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, num_particles=d["particles"], weight_domain="log", measurement_model="bearing", new_landmarks=True,
                     spare_landmarks=d["spare"], record_ids=True, association=association, device=0)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = d["v"], d["w"]
    fs.last_control = tw
    world = np.vstack([uq.TWIN_KNOWN, uq.TWIN_UNKNOWN])
    pose, twice, stats = (0.0, 0.0, 0.0), 0, []
    for s in range(steps):
        pose = truth_step(pose, d["v"], d["w"], d["dt"])
        pk.msgs.Time.set_now(d["dt"] * (s + 1))
        fs.cam_cb(_Scan(wrapped_scan(world, pose)))
        ids = np.asarray(fs.last_ids)
        assert ids.shape == (d["particles"], len(world))
        for row in ids:
            taken = row[row > 0]
            twice += len(taken) - len(np.unique(taken))
        stats.append(fs.association_stats())
    found = int((np.asarray(fs._used) >= 1).sum())
    fs.close()
    return twice, stats, found


def test_the_facade_switches_the_mode_on_and_reports_it(lib):
    """FastSLAM(association="unique") on the demonstration scene of tests/assoc_unique_reference.py: last_ids never claim a landmark
    twice, association_stats() counts the conflicts, the particles find the twin; with "ml" the ids claim the preset twin twice at
    every step, the counters are zero and nobody finds it."""
    twice, stats, found = _facade_drive("unique")
    assert twice == 0 and found >= 8
    assert set(stats[0]) == {"conflicts", "changed", "rematched", "rounds"}
    assert sum(s["conflicts"] for s in stats) >= 16 and sum(s["changed"] for s in stats) >= 16 and max(s["rounds"] for s in stats) >= 2
    twice, stats, found = _facade_drive("ml")
    assert twice >= 16 and found == 0
    assert all(s == dict(conflicts=0, changed=0, rematched=0, rounds=0) for s in stats)

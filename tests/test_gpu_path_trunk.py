"""GPU: the trunk of the path estimate (pk_path_trunk_*, pk_path_settle; pk_k_path_settle.hip; DESIGN.md section 4, "The trunk").

No map and no scan anywhere but in the facade test: DeviceFilter(P, 0), rings built by hand through path_upload with random,
unsorted ancestors, or driven by motion and resample / resample_adaptive.  The reference is path_trunk_reference.py, where the
tolerances are stated; every check prints the errors it measured."""
import random

import numpy as np
import pytest

import path_reference as pr
import path_trunk_reference as pt
from conftest import load_golden
from test_gpu_adaptive import facade_filter, run_facade
from test_gpu_path import raises, same_bits, start_poses
from test_gpu_path_weighted import ring_filter, spread_logw

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1  # PK_ERR_STATE, PK_ERR_INVALID
LIN, LOG, UNIFORM = pt.LIN, pt.LOG, pt.UNIFORM
WEIGHTINGS = (LIN, LOG, UNIFORM)


def trunk_state(f):
    """Ring and trunk figures, and the invariant between them."""
    cap, held, recorded = f.path_shape()
    batch, first, length = f.path_trunk_shape()
    assert first + length == recorded - held, (first, length, recorded, held)
    return cap, held, recorded, batch, first, length


def weighted_rows(f, weighting, logw):
    """pk_path_summary_weighted's rows for this weighting (uniform: the log domain over zero log-weights); the filter's
    log-weights are `logw` again afterwards."""
    if weighting == UNIFORM:
        f.upload_log_weights(np.zeros(f.P))
        sw = f.path_summary_weighted(LOG)
        f.upload_log_weights(logw)
        return sw
    return f.path_summary_weighted(weighting)


def settle_and_check(f, E, weighting, poses, anc, logw, ref, what):
    """One settle of E rows of a ring the host knows (poses, anc: its held rows) against pk_path_summary_weighted's bits, the
    reference, and the ring that must be left.  ref: the Settled of this ring for E rows.  Returns the raw rows."""
    cap, held, recorded, batch, first, length = trunk_state(f)
    assert held == len(anc)
    sw = weighted_rows(f, weighting, logw)
    plain = f.path_summary()
    ring_poses, ring_anc = f.path_download()
    f.path_settle(E, weighting)
    assert trunk_state(f) == (cap, held - E, recorded, batch, first, length + E)
    rows = f.path_trunk_download(first + length, first + length + E)
    assert rows.shape == (E, pt.RES)
    pt.check_rows(rows, ref, what)
    mean, spread, ancestors = f.path_trunk_summary(first + length, first + length + E)
    assert np.array_equal(ancestors, np.column_stack([ref.lo, ref.hi]).reshape(E, 2))
    for t in range(E):
        if ref.final[t]:  # the recorded pose of the one ancestor, no spread
            assert same_bits(mean[t], poses[t][ref.lo[t]]) and spread[t].tolist() == [0.0, 0.0, 0.0, 1.0], (what, t)
        else:             # bit for bit what pk_path_summary_weighted gave for that row
            assert same_bits(mean[t], sw.mean[t]) and same_bits(spread[t], sw.spread[t]), (what, t, mean[t], sw.mean[t])
    # the rows left are the former rows E ..
    after_poses, after_anc = f.path_download()
    assert same_bits(after_poses, ring_poses[E:]) and np.array_equal(after_anc, ring_anc[E:])
    assert same_bits(after_poses, poses[E:]) and np.array_equal(after_anc, anc[E:])
    left = f.path_summary()
    assert same_bits(left.mean, plain.mean[E:]) and same_bits(left.spread, plain.spread[E:])
    assert np.array_equal(left.survivors, plain.survivors[E:]) and left.first_step == plain.first_step + E
    return rows


# ---- 1. hand-built rings: sizes that straddle a wave, a workgroup and the grid (65 793 = 256 x 256 + 257), five rows of a ring of
# eight, none, some and all of them settled
_HAND = {}


def hand_ring(P):
    """The ring of one size and its references for all five rows, made once (the reference of E rows is their first E)."""
    if P not in _HAND:
        rs = np.random.RandomState(7000 + P % 997)
        current = start_poses(rs, P)
        poses = np.stack([start_poses(rs, P)[:, :3] for _ in range(5)])
        anc = rs.randint(0, P, (5, P)).astype(np.int32)
        logw = spread_logw(rs, P)
        _HAND[P] = (current, poses, anc, logw, {w: pt.Settled(poses, anc, current[:, :3], logw, w, 5) for w in WEIGHTINGS})
    return _HAND[P]


@pytest.mark.parametrize("E", [0, 1, 3, 5])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 257, 4097, 65793])
def test_hand_built_rings(lib, P, E):
    current, poses, anc, logw, refs = hand_ring(P)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(current)
    f.path_enable(8)
    raw = {}
    for weighting in WEIGHTINGS + ("log of zeros",):
        f.path_trunk_enable(0)  # a fresh trunk, the same ring
        f.path_trunk_enable(1)
        f.path_upload(poses, anc)
        assert trunk_state(f) == (8, 5, 5, 1, 0, 0)
        if weighting == "log of zeros":
            f.upload_log_weights(np.zeros(P))
            raw[weighting] = settle_and_check(f, E, LOG, poses, anc, np.zeros(P), refs[UNIFORM].first(E),
                                              "P = %d, E = %d, log domain over zero log-weights" % (P, E))
        else:
            f.upload_log_weights(logw)
            raw[weighting] = settle_and_check(f, E, weighting, poses, anc, logw, refs[weighting].first(E),
                                              "P = %d, E = %d, weighting %d" % (P, E, weighting))
    assert same_bits(raw[UNIFORM], raw["log of zeros"])  # uniform: the log domain with every log-weight 0, bit for bit
    f.close()


# ---- 2. the seam and the eight-row turns: a ring of 19 with 23 rows recorded (it wraps); the edge between the walked and the
# reduced rows inside, on and across a turn of eight rows and across the ring's seam; 19 empties the ring
@pytest.mark.parametrize("E", [1, 8, 9, 17, 19])
def test_the_seam_and_the_eight_row_turns(lib, E):
    P, cap, steps = 300, 19, 23
    rs = np.random.RandomState(41)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P) ** 3))
    f.path_enable(cap)
    poses, anc = [], []
    for s in range(steps):
        f.motion(0.3, 0.1, 0.1, z=rs.standard_normal((P, 3)))
        before = f.download_poses()
        a = f.resample(float(rs.uniform(0.0, 1.0)), return_ancestors=True)
        poses.append(before[:, :3].copy())
        anc.append(a.astype(np.int32))
        f.upload_log_weights(spread_logw(rs, P))
    assert f.path_shape() == (cap, cap, steps)
    f.path_trunk_enable(4)  # over a full ring: nothing is settled yet
    assert trunk_state(f) == (cap, cap, steps, 4, steps - cap, 0)
    poses, anc = np.array(poses[-cap:]), np.array(anc[-cap:])
    logw = f.download_log_weights()
    ref = pt.Settled(poses, anc, f.download_poses()[:, :3], logw, LOG, E)
    settle_and_check(f, E, LOG, poses, anc, logw, ref, "wrapped ring, E = %d" % E)
    assert trunk_state(f) == (cap, cap - E, steps, 4, steps - cap, E)
    f.close()


# ---- 3. forced coalescence: rows in front of c final -- the recorded pose of the one ancestor, exactly no variance --, rows from c
# on not; a row with one WEIGHTED lineage but several lineages overall is not final
@pytest.mark.parametrize("c", [1, 3, 5])
def test_forced_coalescence(lib, c):
    P, held = 257, 5
    rs = np.random.RandomState(30 + c)
    f, poses, anc = ring_filter(lib, rs, P, held)
    anc[c - 1][:] = 7
    current = f.download_poses()[:, :3]
    lo, hi = pt.span(anc, P)
    assert np.all(lo[:c] == hi[:c]) and np.all(lo[c:] < hi[c:])  # (the host's view of the ring: nothing below is vacuous)
    spread = spread_logw(rs, P)
    no_zero = spread.copy()
    no_zero[0], no_zero[1] = -np.inf, -0.5  # particle 0, whose lineage is the reference pose, has no weight
    one = np.full(P, -np.inf)
    one[101] = -3.0                         # all weight on one particle
    for logw, weighting, what in ((spread, LIN, "spread"), (spread, LOG, "spread"), (spread, UNIFORM, "spread"), (no_zero, LIN, "particle 0 at 0"),
                                  (no_zero, LOG, "particle 0 at 0"), (one, LIN, "one weighted particle"), (one, LOG, "one weighted particle")):
        f.path_trunk_enable(0)
        f.path_trunk_enable(2)
        f.path_upload(poses, anc)
        f.upload_log_weights(logw)
        ref = pt.Settled(poses, anc, current, logw, weighting, held)
        rows = settle_and_check(f, held, weighting, poses, anc, logw, ref, "coalesced in front of row %d, %s, weighting %d" % (c, what, weighting))
        mean, spread_got, ancestors = f.path_trunk_summary()
        for t in range(c):
            j = int(lo[t])
            assert ancestors[t].tolist() == [j, j]
            assert same_bits(mean[t], poses[t][j]) and same_bits(rows[t, 10:13], poses[t][j])
            assert spread_got[t].tolist() == [0.0, 0.0, 0.0, 1.0] and rows[t, 4:7].tolist() == [0.0, 0.0, 0.0]
        assert np.all(ancestors[c:, 0] < ancestors[c:, 1])  # not final, however the weights lie
        if what == "one weighted particle":  # its lineage's pose (about the reference pose: within TOL, above) without any
            J = pr.lineages(anc, P)          # variance -- and still not final
            for t in range(c, held):
                assert abs(mean[t, 0] - poses[t][J[t][101], 0]) <= pt.TOL * abs(mean[t, 0])
                assert spread_got[t, :3].tolist() == [0.0, 0.0, 0.0]
    f.close()


# ---- 4. the automatic mode: the scene of path_trunk_reference.AutoScene; the host keeps the whole history
def drive(lib, batch, mode, check=True, P=1025, cap=6, steps=24):
    """mode None: motion and resample; LIN / LOG: resample_adaptive in that domain, kept (threshold 0) and resampled (2) in turn,
    other weights uploaded behind every resample.  Returns the raw trunk rows and how many of them are final."""
    sc = pt.AutoScene(P, steps, pt.AUTO_SEED)
    rs = np.random.RandomState(77)  # (the weights uploaded behind the adaptive resamples)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(np.random.RandomState(5), P, sc.start_weights))
    f.path_enable(cap)
    f.path_trunk_enable(batch)
    poses, anc, kept_rows = [], [], np.empty((0, pt.RES))
    for s in range(steps):
        f.motion(0.3, 0.1, 0.1, z=sc.z[s])
        now = f.download_poses()
        for i, w in sc.heavy[s]:
            f.upload_pose(i, np.append(now[i, :3], w))
        before = f.download_poses()
        if mode is None:
            a = f.resample(sc.u[s], return_ancestors=True)
        else:
            a = f.resample_adaptive(sc.u[s], 0.0 if s % 2 == 0 else 2.0, domain=mode, return_ancestors=True)
            assert f.resample_stats().resampled == (s % 2 == 1)
        poses.append(before[:, :3].copy())
        anc.append(a.astype(np.int32))
        logw = f.download_log_weights()  # the new generation's: what a settle behind this record took
        _, held, recorded, _, first, length = trunk_state(f)
        assert held < cap and recorded == s + 1 and first == 0
        if length > kept_rows.shape[0]:  # this step settled: `batch` rows of the ring that was full behind its record
            assert length == kept_rows.shape[0] + batch and held == cap - batch
            new = f.path_trunk_download(length - batch, length)
            if check:
                ref = pt.Settled(np.array(poses[-cap:]), np.array(anc[-cap:]), f.download_poses()[:, :3], logw,
                                 UNIFORM if mode is None else mode, batch)
                pt.check_rows(new, ref, "batch %d, mode %s, step %d" % (batch, mode, s))
            kept_rows = np.concatenate([kept_rows, new])
        else:
            assert held == (s + 1) - length
        assert same_bits(f.path_trunk_download(), kept_rows)  # what was settled stays as it was settled
        if mode is not None and s % 2 == 1:
            f.upload_log_weights(spread_logw(rs, P))
    if check:
        mean, spread, ancestors = f.path_trunk_summary()
        ref_mean, ref_spread, ref_anc = pt.summary_of(kept_rows)
        assert np.array_equal(ancestors, ref_anc)
        fin = ref_anc[:, 0] == ref_anc[:, 1]
        assert same_bits(mean[fin], ref_mean[fin]) and same_bits(spread[fin], ref_spread[fin])
        assert np.allclose(mean, ref_mean, rtol=1e-14, atol=1e-14) and np.allclose(spread, ref_spread, rtol=1e-14, atol=0.0)
    f.close()
    return kept_rows, int(np.sum(kept_rows[:, 8] == kept_rows[:, 9]))


@pytest.mark.parametrize("mode", [None, LIN, LOG])
@pytest.mark.parametrize("batch", [1, 2, 6])
def test_automatic_mode(lib, batch, mode):
    rows, n_final = drive(lib, batch, mode)
    assert rows.shape[0] == {1: 19, 2: 20, 6: 24}[batch]
    print("batch %d, mode %s: %d of %d settled rows final" % (batch, mode, n_final, rows.shape[0]))
    assert 0 < n_final < rows.shape[0]  # both kinds were checked


# ---- 5. the same bits twice
def test_the_same_bits_twice(lib):
    for mode in (None, LOG):
        a, _ = drive(lib, 2, mode, check=False)
        b, _ = drive(lib, 2, mode, check=False)
        assert a.shape == (20, pt.RES) and same_bits(a, b)


# ---- 6. growth and memory: the trunk passes 1 024 and 2 048 rows; what it holds is counted and given back
def test_growth_and_memory(lib):
    P, cap, batch = 64, 4, 2
    rs = np.random.RandomState(6)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P)))
    f.resample(0.5)  # (whatever a resample and an upload of weights allocate when first called is held before the figures are taken)
    f.upload_log_weights(rs.uniform(-2.0, 0.0, P))
    b0 = f.device_bytes()
    f.path_enable(cap)
    b1 = f.device_bytes()
    f.path_trunk_enable(batch)
    b2 = f.device_bytes()
    assert b2 - b1 >= 1024 * pt.RES * 8 + 12 * P  # the rows, and the settle scratch
    kept, steps = {}, 0
    while f.path_trunk_shape()[2] <= 2048:
        if steps % 3 == 0:
            f.upload_log_weights(rs.uniform(-2.0, 0.0, P))
        f.resample(float(rs.uniform(0.0, 1.0)))
        steps += 1
        _, held, recorded, _, first, length = trunk_state(f)
        assert recorded == steps and first == 0 and cap - batch <= held < cap or steps < cap
        if length in (1024, 2048) and length not in kept:  # full to the last row: the next settle doubles it
            kept[length] = (f.path_trunk_download(), f.device_bytes())
    assert sorted(kept) == [1024, 2048]
    assert kept[1024][1] == b2 and kept[2048][1] - b2 == 1024 * pt.RES * 8 and f.device_bytes() - b2 == 3 * 1024 * pt.RES * 8
    rows = f.path_trunk_download()
    assert rows.shape[0] == f.path_trunk_shape()[2] > 2048
    assert same_bits(rows[:1024], kept[1024][0]) and same_bits(rows[:2048], kept[2048][0])  # intact across both doublings
    assert np.all(rows[:, 8] <= rows[:, 9]) and np.all(rows[:, 7] == P)
    f.path_trunk_enable(0)
    assert f.device_bytes() == b1
    raises(lib, STATE, f.path_trunk_shape)
    f.path_trunk_enable(batch)
    assert f.device_bytes() == b2 and trunk_state(f)[3:] == (batch, steps - f.path_shape()[1], 0)
    f.path_enable(0)
    assert f.device_bytes() == b0
    f.close()


# ---- 7. off is off; refusals and argument errors, with nothing changed
def test_off_is_off_and_refusals(lib):
    P, cap = 64, 4
    rs = np.random.RandomState(8)
    f = lib.DeviceFilter(P, 0)
    f.upload_poses(start_poses(rs, P, rs.uniform(0.1, 1.0, P)))
    assert "pk_path_enable" in raises(lib, STATE, f.path_trunk_enable, 1)  # no ring
    f.path_enable(cap)
    poses, anc = [], []
    for s in range(cap + 3):  # a ring without a trunk overwrites as before
        f.motion(0.3, 0.1, 0.1, z=rs.standard_normal((P, 3)))
        before = f.download_poses()
        a = f.resample(float(rs.uniform(0.0, 1.0)), return_ancestors=True)
        poses.append(before[:, :3].copy())
        anc.append(a.astype(np.int32))
        f.upload_log_weights(rs.uniform(-2.0, 0.0, P))
        assert f.path_shape() == (cap, min(s + 1, cap), s + 1)
    got_poses, got_anc = f.path_download()
    assert same_bits(got_poses, np.array(poses[-cap:])) and np.array_equal(got_anc, np.array(anc[-cap:]))
    rows13 = np.zeros((1, pt.RES))
    for fn, args in ((f.path_settle, (1,)), (f.path_trunk_shape, ()), (f.path_trunk_download, (0, 0)), (f.path_trunk_upload, (rows13, 0)),
                     (f.path_trunk_summary, (0, 0))):
        assert "pk_path_trunk_enable" in raises(lib, STATE, fn, *args)
    for bad in (-1, cap + 1):
        raises(lib, INVALID, f.path_trunk_enable, bad)
    raises(lib, STATE, f.path_trunk_shape)

    # switched on over the full ring: it stays full, and the next record first settles `batch` rows by the generation it records
    f.path_trunk_enable(2)
    assert trunk_state(f) == (cap, cap, cap + 3, 2, 3, 0)
    for fn, args in ((f.path_settle, (-1,)), (f.path_settle, (cap + 1,)), (f.path_settle, (1, 3)), (f.path_settle, (1, -1)),
                     (f.path_trunk_download, (2, 3)), (f.path_trunk_download, (3, 4)), (f.path_trunk_summary, (3, 4)),
                     (f.path_trunk_summary, (4, 3))):
        raises(lib, INVALID, fn, *args)
    assert "holds" in raises(lib, STATE, f.path_trunk_upload, rows13, 0)  # the ring holds rows
    assert trunk_state(f) == (cap, cap, cap + 3, 2, 3, 0)
    f.path_settle(0)  # nothing: fine
    assert f.path_trunk_download().shape == (0, pt.RES) and f.path_trunk_summary()[0].shape == (0, 3)
    f.motion(0.3, 0.1, 0.1, z=rs.standard_normal((P, 3)))
    before = f.download_poses()
    a = f.resample(float(rs.uniform(0.0, 1.0)), return_ancestors=True)
    assert trunk_state(f) == (cap, cap - 1, cap + 4, 2, 3, 2)
    pt.check_rows(f.path_trunk_download(), pt.Settled(np.array(poses[-cap:]), np.array(anc[-cap:]), before[:, :3], None, UNIFORM, 2),
                  "a record into a full ring")
    poses.append(before[:, :3].copy())
    anc.append(a.astype(np.int32))
    got_poses, got_anc = f.path_download()
    assert same_bits(got_poses, np.array(poses[-3:])) and np.array_equal(got_anc, np.array(anc[-3:]))

    # pk_path_upload must continue the trunk; a full ring settles `batch` rows at once, uniformly
    kept = f.path_trunk_download()
    up_poses, up_anc = np.array(poses[-cap:]), np.array(anc[-cap:])
    raises(lib, INVALID, f.path_upload, up_poses[:2], up_anc[:2], cap + 4 + 1)  # steps 7, 8 behind a trunk that ends at 5
    assert trunk_state(f) == (cap, cap - 1, cap + 4, 2, 3, 2) and same_bits(f.path_trunk_download(), kept)
    f.path_upload(up_poses[1:], up_anc[1:], cap + 4)  # steps 5, 6, 7: they follow
    assert trunk_state(f) == (cap, 3, cap + 4, 2, 3, 2)
    # bad trunk rows: lo > hi, outside [0, P), not whole
    f.path_upload(np.empty((0, P, 3)), np.empty((0, P), dtype=np.int32), cap + 4 - 3)
    assert trunk_state(f)[1] == 0
    for lo, hi in ((5, 4), (-1, 3), (0, P), (1.5, 2)):
        bad = kept.copy()
        bad[1, 8:10] = (lo, hi)
        raises(lib, INVALID, f.path_trunk_upload, bad, 3)
    assert same_bits(f.path_trunk_download(), kept)
    f.path_trunk_upload(kept[:1], 10)  # replaces the trunk and sets the counter
    assert trunk_state(f) == (cap, 0, 11, 2, 10, 1) and same_bits(f.path_trunk_download(), kept[:1])
    f.path_upload(up_poses, up_anc, 11 + cap)  # a full ring: two rows settled at once
    assert trunk_state(f) == (cap, cap - 2, 11 + cap, 2, 10, 3)
    pt.check_rows(f.path_trunk_download(11, 13), pt.Settled(up_poses, up_anc, f.download_poses()[:, :3], None, UNIFORM, 2), "a full upload")
    # an empty trunk takes its first step from the upload
    f.path_trunk_enable(0)
    f.path_trunk_enable(1)
    f.path_upload(up_poses[:2], up_anc[:2], 40)
    assert trunk_state(f) == (cap, 2, 40, 1, 38, 0)
    # pk_upload_poses empties ring and trunk; pk_path_enable starts without a trunk
    f.path_settle(1)
    assert trunk_state(f) == (cap, 1, 40, 1, 38, 1)
    f.upload_poses(start_poses(rs, P))
    assert trunk_state(f) == (cap, 0, 40, 1, 40, 0)
    f.path_enable(cap)
    raises(lib, STATE, f.path_trunk_shape)
    f.close()


# ---- 8. the facade: FastSLAM(record_path=4, settle_path=2)
def test_facade(tmp_path):
    import parakeet_slam_amd as pk
    from parakeet_slam_amd import msgs, path as pkpath

    pk.msgs = msgs
    g = load_golden("step_small")
    with pytest.raises(ValueError, match="one GPU"):
        pk.FastSLAM([], num_particles=512, devices=[0, 1], record_path=4, settle_path=2)
    for kw in (dict(settle_path=2), dict(record_path=4, settle_path=5), dict(record_path=4, settle_path=-1)):
        with pytest.raises(ValueError, match="settle_path"):
            pk.FastSLAM([], num_particles=8, **kw)

    def seeded(**kw):
        np.random.seed(3)
        random.seed(3)
        msgs.Time.set_now(0.0)
        return facade_filter(pk, g, **kw)

    fs = seeded(record_path=4, settle_path=2)
    run_facade(pk, fs, g, 10)
    full = fs.full_path()
    assert isinstance(full, pkpath.FullPath)
    assert fs._filter.path_shape()[2] == 10 and full.steps().tolist() == list(range(11))  # steps 0 .. recorded, no gap
    held = fs._filter.path_shape()[1]
    assert full.in_trunk.tolist() == [True] * (10 - held) + [False] * (held + 1) and 2 <= held < 4
    ring = fs.path_summary()
    assert same_bits(full.mean[10 - held:], ring.mean) and np.array_equal(full.final[10 - held:], ring.survivors == 1)
    assert np.all(full.ancestors[10 - held:] == -1) and np.all(full.ancestors[:10 - held] >= 0)
    assert not fs.full_path("weights").final[10 - held:].any()
    assert len(pkpath.as_poses(full)) == 11
    true_default = seeded(record_path=8, settle_path=True)
    assert true_default._filter.path_trunk_shape()[0] == 2
    true_default.close()
    plain = seeded(record_path=4)  # without settle_path: path_summary in FullPath's form
    run_facade(pk, plain, g, 3)
    p_full, p_sum = plain.full_path(), plain.path_summary()
    assert same_bits(p_full.mean, p_sum.mean) and not p_full.in_trunk.any() and p_full.first_step == p_sum.first_step
    plain.close()

    snap = str(tmp_path / "snap.npz")
    fs.save_state(snap)
    d = np.load(snap)
    assert d["path_trunk_rows"].shape == (10 - held, pt.RES) and int(d["path_trunk_first"]) == 0
    other = seeded(record_path=4, settle_path=2)
    other.load_state(snap)

    def same_path(a, b):
        return (same_bits(a.mean, b.mean) and same_bits(a.spread, b.spread) and np.array_equal(a.final, b.final)
                and np.array_equal(a.in_trunk, b.in_trunk) and np.array_equal(a.ancestors, b.ancestors) and a.first_step == b.first_step)

    assert same_path(other.full_path(), full)
    outs = []
    for f in (fs, other):
        np.random.seed(9)
        random.seed(9)
        f.last_update = msgs.Time(0.1 * 10)
        run_facade(pk, f, g, 3, first=10)
        outs.append(f.full_path())
    assert outs[0].steps().tolist() == list(range(14)) and same_path(outs[0], outs[1])
    fs.close()
    other.close()

"""CPU: the trunk's reference (path_trunk_reference.py) against the definitions it restates, and the host classes the trunk's
figures arrive in (parakeet_slam_amd.path.FullPath, as_poses)."""
import numpy as np
import pytest

import path_reference as pr
import path_trunk_reference as pt
import path_weighted_reference as pw


def random_ring(rs, P, T, coalesce_at=None):
    poses = np.column_stack([rs.uniform(10, 20, T * P), rs.uniform(-5, 5, T * P), rs.uniform(-0.6, 0.6, T * P)]).reshape(T, P, 3)
    anc = rs.randint(0, P, (T, P)).astype(np.int32)
    if coalesce_at is not None:
        anc[coalesce_at][:] = 7 % P
    current = np.column_stack([rs.uniform(10, 20, P), rs.uniform(-5, 5, P), rs.uniform(-0.6, 0.6, P)])
    return poses, anc, current


@pytest.mark.parametrize("P,T,coalesce_at", [(1, 3, None), (2, 9, None), (65, 6, None), (30, 200, None), (65, 6, 0), (65, 6, 3), (300, 12, 11)])
def test_final_rows_are_a_prefix(P, T, coalesce_at):
    rs = np.random.RandomState(P + T)
    poses, anc, current = random_ring(rs, P, T, coalesce_at)
    fin = pt.final_rows(anc, P)
    assert fin.shape == (T + 1,)
    n = int(fin.sum())
    assert fin[:n].all() and not fin[n:].any(), fin.tolist()  # j_{t-1} is a function of j_t
    assert fin[T] == (P == 1)
    if coalesce_at is not None:
        assert n >= coalesce_at + 1
    lo, hi = pt.span(anc, P)
    assert np.array_equal(fin, pr.survivors(anc, P) == 1)
    assert np.all(lo <= hi) and lo.min() >= 0 and hi.max() < P
    if T == 200:
        assert 0 < n < T  # random maps of 30 particles coalesce within some 60 rows: both kinds are present


@pytest.mark.parametrize("weighting", [pt.LIN, pt.LOG, pt.UNIFORM])
def test_a_final_rows_estimate_is_its_ancestors_pose(weighting):
    P, T, c = 65, 6, 3
    rs = np.random.RandomState(5)
    poses, anc, current = random_ring(rs, P, T, coalesce_at=c - 1)
    logw = rs.uniform(-30.0, 0.0, P)
    logw[rs.permutation(P)[:P // 10]] = -np.inf
    ref = pt.Settled(poses, anc, current, logw, weighting, T)
    assert ref.final[:c].all() and not ref.final[c:].any()
    J = pr.lineages(anc, P)
    for t in range(c):
        assert ref.lo[t] == ref.hi[t] == J[t][0]
        assert np.array_equal(ref.pose[t], poses[t][J[t][0]])
        assert ref.mean[t, 0] == ref.pose[t, 0] and ref.mean[t, 1] == ref.pose[t, 1]
        assert pr.angle_diff(ref.mean[t, 2], ref.pose[t, 2]) <= 1e-15
        assert ref.spread[t, :3].tolist() == [0.0, 0.0, 0.0] and abs(ref.spread[t, 3] - 1.0) <= 1e-15
    assert np.all(ref.spread[c:, [0, 2]] > 0.0)
    # a settle of E rows leaves the rows E .. of the ring
    part = pt.Settled(poses, anc, current, logw, weighting, 2)
    assert np.array_equal(part.ring_poses, poses[2:]) and np.array_equal(part.ring_anc, anc[2:]) and part.E == 2
    assert np.array_equal(part.mean, ref.mean[:2])
    again = ref.first(2)
    assert again.E == 2 and np.array_equal(again.ring_poses, part.ring_poses) and np.array_equal(again.ring_anc, part.ring_anc)
    for name in ("lo", "hi", "final", "pose", "mean", "spread"):
        assert np.array_equal(getattr(again, name), getattr(part, name)), name
    assert again.s1 == part.s1
    # uniform is the log domain with every log-weight 0
    if weighting == pt.UNIFORM:
        mean, spread, n_eff = pw.summary(poses, anc, current, np.zeros(P), True)
        assert np.array_equal(mean[:T], ref.mean) and np.array_equal(spread[:T], ref.spread) and n_eff == P and ref.s1 == P


def test_raw_rows_round_trip_through_the_check():
    """Rows built from the reference's own figures pass check_rows; a wrong ancestor, pose bit or moment does not."""
    P, T = 65, 5
    rs = np.random.RandomState(8)
    poses, anc, current = random_ring(rs, P, T, coalesce_at=1)
    logw = rs.uniform(-3.0, 0.0, P)
    ref = pt.Settled(poses, anc, current, logw, pt.LOG, 4)
    r = ref.spread[:, 3] * ref.s1
    rows = np.column_stack([ref.mean[:, 0], ref.mean[:, 1], r * np.sin(ref.mean[:, 2]), r * np.cos(ref.mean[:, 2]), ref.spread[:, 0],
                            ref.spread[:, 1], ref.spread[:, 2], np.full(4, ref.s1), ref.lo, ref.hi, ref.pose])
    pt.check_rows(rows, ref, "round trip")
    mean, spread, ancestors = pt.summary_of(rows)
    assert np.array_equal(mean[:2], ref.pose[:2]) and spread[:2].tolist() == [[0.0, 0.0, 0.0, 1.0]] * 2
    assert np.array_equal(ancestors, np.column_stack([ref.lo, ref.hi]))
    for col, delta in ((8, 1.0), (12, 1e-16), (4, 1e-9), (0, 1e-9)):
        bad = rows.copy()
        bad[3, col] += delta if col != 12 else np.spacing(bad[3, col])
        with pytest.raises(AssertionError):
            pt.check_rows(bad, ref, "spoiled column %d" % col)


def test_full_path_assembly_and_as_poses():
    from parakeet_slam_amd import path as pkpath

    assert pkpath.TRUNK_RES == pt.RES
    rs = np.random.RandomState(3)
    held = 3
    ring = pkpath.PathSummary(rs.uniform(0, 1, (held + 1, 3)), rs.uniform(0, 1, (held + 1, 4)), [1, 1, 5, 9], first_step=7)
    t_mean, t_spread = rs.uniform(0, 1, (4, 3)), rs.uniform(0, 1, (4, 4))
    t_anc = np.array([[2, 2], [0, 0], [1, 6], [4, 4]])
    full = pkpath.FullPath.assemble((t_mean, t_spread, t_anc, 3), ring, ring.survivors == 1)
    assert full.first_step == 3 and full.steps().tolist() == list(range(3, 11))
    assert full.mean.shape == (8, 3) and full.spread.shape == (8, 4)
    assert np.array_equal(full.mean[:4], t_mean) and np.array_equal(full.mean[4:], ring.mean)
    assert np.array_equal(full.spread[:4], t_spread) and np.array_equal(full.spread[4:], ring.spread)
    assert full.final.tolist() == [True, True, False, True, True, True, False, False] and full.final.dtype == bool
    assert full.in_trunk.tolist() == [True] * 4 + [False] * 4 and full.in_trunk.dtype == bool
    assert full.ancestors.tolist() == t_anc.tolist() + [[-1, -1]] * 4
    track = pkpath.as_poses(full)
    assert len(track) == 8 and all(type(v) is float for p in track for v in p)
    assert track[0] == tuple(t_mean[0]) and track[-1] == tuple(ring.mean[-1])
    assert "in_trunk=4" in repr(full)
    # without a trunk: the summary in FullPath's form; a weighted summary, whose rows are reported not final
    plain = pkpath.FullPath.assemble(None, ring, ring.survivors == 1)
    assert plain.first_step == 7 and not plain.in_trunk.any() and plain.final.tolist() == [True, True, False, False]
    assert np.array_equal(plain.mean, ring.mean) and np.all(plain.ancestors == -1)
    w = pkpath.WeightedPathSummary(ring.mean, ring.spread, 2.5, first_step=7)
    fw = pkpath.FullPath.assemble((t_mean, t_spread, t_anc, 3), w, np.zeros(held + 1, dtype=bool))
    assert fw.final.tolist() == [True, True, False, True] + [False] * 4
    with pytest.raises(ValueError, match="does not meet"):  # a gap between trunk and ring
        pkpath.FullPath.assemble((t_mean, t_spread, t_anc, 2), ring, ring.survivors == 1)


@pytest.mark.parametrize("batch", [1, 2, 6])
def test_the_automatic_scene_settles_final_rows_and_others(batch):
    """The scene test_gpu_path_trunk drives (P = 1025, a ring of 6, 24 steps), resampled here by the exact systematic resampler:
    for every batch some settled rows are final and some are not, so neither kind of check there can pass vacuously."""
    from resample_reference import exact_ancestors

    P, cap, steps = 1025, 6, 24
    sc = pt.AutoScene(P, steps, seed=pt.AUTO_SEED)
    w, anc = sc.start_weights.copy(), []
    for s in range(steps):
        for i, heavy in sc.heavy[s]:
            w[i] = heavy
        anc.append(exact_ancestors(np.log(w), sc.u[s], False)[0])
        w = np.ones(P)
    kinds = pt.settled_kinds(anc, P, cap, batch)
    assert [k[0] for k in kinds] == list(range(len(kinds)))  # the settled steps follow one another from 0
    assert len(kinds) == {1: 19, 2: 20, 6: 24}[batch]
    n_final = sum(k[1] for k in kinds)
    print("batch %d: %d of %d settled rows final" % (batch, n_final, len(kinds)))
    assert 0 < n_final < len(kinds), kinds


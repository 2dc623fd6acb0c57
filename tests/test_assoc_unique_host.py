"""CPU: unique data association (pk_assoc_unique; DESIGN.md section 4, "Unique association") -- the rule's own properties on random
matrices with planted ties, the oracle mixin on all three measurement models, the demonstration scene that justifies the feature
(figures recorded in tests/golden/assoc_unique_twin_scene.json), and the facade's refusals.  No GPU."""
import json
import os

import numpy as np
import pytest

import assoc_unique_reference as uq
from assoc_unique_reference import deferred_acceptance, ml_ids, unique_ids, uniquely
from bearing_model_reference import BearingOracle, wrapped_scan
from conftest import GOLDEN
from oracle.fastslam_oracle import OracleFilter, synthetic_scan, synthetic_world
from range_bearing_reference import RangeBearingOracle


def _textbook(prob):
    """Gale-Shapley as the textbooks have it, one free blob at a time, no table tricks: blobs propose down their lists (p
    descending, landmark ascending), a landmark prefers p descending, blob ascending."""
    p = np.where(np.isnan(prob), 0.0, prob)
    B, L = p.shape
    lists = []
    for b in range(B):
        ls = [l for l in range(L) if p[b, l] > 0.0]
        lists.append(sorted(ls, key=lambda l: (-p[b, l], l)))
    nxt, holder, free = [0] * B, {}, list(range(B))
    while free:
        b = free.pop()
        if nxt[b] >= len(lists[b]):
            continue
        l = lists[b][nxt[b]]
        nxt[b] += 1
        h = holder.get(l)
        if h is None or (p[b, l], -b) > (p[h, l], -h):
            holder[l] = b
            if h is not None:
                free.append(h)
        else:
            free.append(b)
    ids = np.zeros(B, dtype=np.int32)
    for l, b in holder.items():
        ids[b] = l + 1
    return ids


def _random_matrix(rs, B, L, density, ties):
    p = rs.uniform(0.0, 1.0, (B, L)) * (rs.uniform(size=(B, L)) < density)
    p *= 10.0 ** rs.uniform(-250, 0, (B, 1))  # rows of very different scale, as scans have them
    for _ in range(ties):  # planted ties: equal entries in a row, in a column, and a duplicated row / column
        b, l, b2, l2 = rs.randint(B), rs.randint(L), rs.randint(B), rs.randint(L)
        kind = rs.randint(4)
        if kind == 0:
            p[b, l2] = p[b, l]
        elif kind == 1:
            p[b2, l] = p[b, l]
        elif kind == 2:
            p[b2] = p[b]
        else:
            p[:, l2] = p[:, l]
    if rs.uniform() < 0.3:
        p[rs.randint(B), rs.randint(L)] = np.nan
    return p


@pytest.mark.parametrize("seed", range(6))
def test_greedy_is_deferred_acceptance_is_the_textbook_stable_matching(seed):
    rs = np.random.RandomState(100 + seed)
    conflicts = 0
    for _ in range(60):
        B, L = rs.randint(1, 14), rs.randint(1, 14)
        p = _random_matrix(rs, B, L, rs.choice([0.15, 0.5, 1.0]), rs.randint(0, 6))
        want = unique_ids(p)
        got, passes = deferred_acceptance(p)
        assert np.array_equal(got, want), (p, got, want)
        assert np.array_equal(_textbook(p), want), p
        assert 1 <= passes <= B + 1
        taken = want[want > 0]
        assert len(np.unique(taken)) == len(taken)  # no landmark twice
        clean = np.where(np.isnan(p), 0.0, p)
        assert all(clean[b, want[b] - 1] > 0.0 for b in range(B) if want[b])  # only candidates are taken
        ml = ml_ids(p)
        if len(np.unique(ml[ml > 0])) == len(ml[ml > 0]):
            assert np.array_equal(want, ml) and passes == 1  # conflict-free: the argmax ids, element for element
        else:
            conflicts += 1
            assert passes >= 2
    assert conflicts >= 15


def test_the_tie_order_is_lower_blob_then_lower_landmark():
    p = np.zeros((3, 3))
    p[0, 1] = p[2, 1] = 0.5          # two identical blobs want landmark 2: the lower blob keeps it
    assert list(unique_ids(p)) == [2, 0, 0]
    p = np.zeros((2, 3))
    p[:, 1] = p[:, 2] = 0.5          # two identical landmarks, two identical blobs: blob 0 the lower, blob 1 the next
    assert list(unique_ids(p)) == [2, 3]
    assert list(deferred_acceptance(p)[0]) == [2, 3]


def test_a_displacement_chain_takes_its_passes_and_an_exhausted_blob_ends_unmatched():
    # blob 2 loses landmark 1 to blob 0 and displaces blob 1 from landmark 2, who displaces blob 3 from landmark 3, who has no other
    p = np.array([[0.9, 0.0, 0.0],
                  [0.0, 0.6, 0.5],
                  [0.8, 0.7, 0.0],
                  [0.0, 0.0, 0.4]])
    ids, passes = deferred_acceptance(p)
    assert list(ids) == [1, 3, 2, 0] and list(unique_ids(p)) == [1, 3, 2, 0]
    assert passes == 4


def _world(L, B, seed):
    means, covs = synthetic_world(L, seed=seed)
    rs = np.random.RandomState(seed)
    return means, covs, rs


@pytest.mark.parametrize("model", ["reference", "bearing", "range"])
def test_the_mixin_gives_every_oracle_the_rule(model):
    L, P = 12, 6
    means, covs, rs = _world(L, L, 5)
    cls = {"reference": OracleFilter, "bearing": BearingOracle, "range": RangeBearingOracle}[model]
    a, b = cls(P, means, covs), uniquely(cls(P, means, covs))
    for o in (a, b):
        o.x[:] = rs.normal(0, 0.05, P) if o is a else a.x
        o.y[:] = 0.0
        o.h[:] = 0.0
    pose = (0.0, 0.0, 0.0)
    scan = synthetic_scan(means, pose) if model == "reference" else wrapped_scan(means, pose)
    blobs = np.vstack([scan, scan[[3, 3, 7]]])  # landmark 4 is seen three times, landmark 8 twice
    blobs[-3:, 0] += [0.004, -0.006, 0.003]
    kw = {}
    if model == "range":
        rho = np.hypot(means[:, 0], means[:, 1])
        kw = dict(ranges=np.concatenate([rho, [np.nan, rho[3] + 0.1, np.nan]]), variances=np.full(len(blobs), 0.04))
    ml = a.associate(blobs, **kw)
    un = b.associate(blobs, **kw)
    assert (ml[:, [3, L, L + 1]] == 4).all() and (ml[:, [7, L + 2]] == 8).all()  # the maximum-likelihood ids claim them twice
    for i in range(P):
        taken = un[i][un[i] > 0]
        assert len(np.unique(taken)) == len(taken)
        assert (un[i] == 4).sum() == 1 and (un[i] == 8).sum() == 1
    same = [c for c in range(len(blobs)) if c not in (3, 7, L, L + 1, L + 2)]
    assert np.array_equal(un[:, same], ml[:, same])
    assert b.unique_stats[0] == P and b.unique_stats[1] >= 3 * P and b.unique_stats[3] >= 2
    # a scan without a conflict: the ids of the plain oracle, and nothing counted
    assert np.array_equal(b.associate(scan, **({k: v[:L] for k, v in kw.items()})), a.associate(scan, **({k: v[:L] for k, v in kw.items()})))
    assert b.unique_stats == (0, 0, 0, 1)


def test_the_demonstration_scene_unique_finds_the_twin_and_ml_never_does():
    """The scene of assoc_unique_reference.twin_scene_run: an unknown landmark of a preset landmark's colour, 2 m beside it, both
    inside one bearing gate for the whole drive.  Maximum likelihood matches both blobs to the preset landmark at every step -- it is
    updated twice a scan and pulled towards the twin, and the twin's blob is never unmatched, so no particle ever stores a reading of
    it.  Unique association leaves one of the two blobs unmatched; the twin is triangulated and promoted within the drive.  Only
    that qualitative outcome is asserted; the figures are in tests/golden/assoc_unique_twin_scene.json."""
    recorded = json.load(open(os.path.join(GOLDEN, "assoc_unique_twin_scene.json")))
    seed = recorded["runs"][0]["seed"]
    steps = uq.TWIN_DRIVE["steps"]
    ml, un = uq.twin_scene_run("ml", seed), uq.twin_scene_run("unique", seed)
    print(json.dumps([ml, un]))
    assert ml["promoted_at_step"] is None and ml["particles_with_the_twin"] == 0 and ml["readings_stored"] == 0
    assert ml["known_updates"] == 2 * steps  # two importance factors and two updates of one landmark per scan
    assert un["promoted_at_step"] is not None and un["promoted_at_step"] < steps
    assert un["particles_with_the_twin"] == uq.TWIN_DRIVE["particles"]
    assert un["known_updates"] == steps  # at most one update per scan
    assert un["known_error"] < ml["known_error"]


# ---------------------------------------------------------------------------------------------------------------- the facade's refusals
def test_the_facade_refuses_what_the_mode_does_not_cover():
    from parakeet_slam_amd.core import FastSLAM, _check_association
    from parakeet_slam_amd.multi import ShardedFastSLAM

    assert _check_association("ml", "motion", None) == "ml" and _check_association("unique", "motion", [0]) == "unique"
    with pytest.raises(ValueError, match="'ml' \\(default\\) or 'unique'"):
        FastSLAM([], association="hungarian")
    with pytest.raises(ValueError, match="one GPU"):
        FastSLAM([], devices=[0, 1], association="unique")
    with pytest.raises(ValueError, match="settles its own"):
        FastSLAM([], measurement_model="bearing", proposal="measurement", association="unique")
    with pytest.raises(ValueError, match="one GPU"):
        ShardedFastSLAM([], devices=(0, 1), association="unique")
    with pytest.raises(ValueError, match="'ml' \\(default\\) or 'unique'"):
        ShardedFastSLAM([], devices=(0, 1), association="hungarian")

"""Unique data association (pk_assoc_unique; DESIGN.md section 4, "Unique association") in NumPy, float64 -- the yardstick of
tests/test_assoc_unique_host.py and tests/test_gpu_assoc_unique.py.  TEST INFRASTRUCTURE ONLY.

The rule, per particle, on the (B, L) matrix of match probabilities the oracles already form: the pairs with p > 0 (a NaN is no
pair) are walked by p descending, then blob ascending, then landmark ascending, and a pair is taken iff neither its blob nor its
landmark has been.  ids[b] = the taken landmark + 1, or 0.

    unique_ids(prob)            the rule itself, by one sort
    deferred_acceptance(prob)   the device's formulation: blobs propose down their own lists, landmarks keep the best proposal, a
                                proposal that cannot beat what a landmark holds is never made -- (ids, passes)
    UniqueAssociation           a mixin that gives an oracle filter the rule in place of its per-blob argmax
    uniquely(o)                 ... applied to a live oracle (an OracleFilter of any model, or a growing oracle's filter)
"""
import numpy as np

import bearing_model_reference as bearing
import range_bearing_reference as rb
from oracle.fastslam_oracle import GrowingOracle, OracleFilter, probability_of_match as reference_probability


def _clean(prob):
    p = np.asarray(prob, dtype=np.float64)
    return np.where(np.isnan(p), 0.0, p)


def ml_ids(prob):
    """The per-blob argmax (strict '>' from 0: the earliest landmark among equals, 0 where nothing is positive)."""
    p = _clean(prob)
    B, L = p.shape
    if L == 0 or B == 0:
        return np.zeros(B, dtype=np.int32)
    best = np.argmax(p, axis=1)
    return np.where(p[np.arange(B), best] > 0.0, best + 1, 0).astype(np.int32)


def unique_ids(prob):
    """(B, L) probabilities -> ids (B,) by the greedy rule."""
    p = _clean(prob)
    B, L = p.shape
    ids = np.zeros(B, dtype=np.int32)
    bb, ll = np.nonzero(p > 0.0)
    if bb.size == 0:
        return ids
    order = np.lexsort((ll, bb, -p[bb, ll]))  # (last key first) p descending, blob ascending, landmark ascending
    taken = np.zeros(L, dtype=bool)
    left = B
    for k in order:
        b, l = bb[k], ll[k]
        if ids[b] == 0 and not taken[l]:
            ids[b] = l + 1
            taken[l] = True
            left -= 1
            if left == 0:
                break
    return ids


def deferred_acceptance(prob):
    """The same matching the way the device reaches it -> (ids, passes).  Every pass: each landmark keeps the largest key among the
    blobs standing at it (the lowest blob among equals); a blob that is not kept goes to the best pair strictly behind its own in its
    list that beats what the landmark holds (the tables only rise: what cannot win now never can), or ends 0.  passes counts the
    claims passes; 1: the maximum-likelihood ids claimed no landmark twice."""
    p = _clean(prob)
    B, L = p.shape
    cur = ml_ids(p).astype(np.int64) - 1
    best = np.zeros(L)
    win = np.full(L, -1, dtype=np.int64)
    passes = 0
    while True:
        active = np.nonzero(cur >= 0)[0]
        for b in active:
            best[cur[b]] = max(best[cur[b]], p[b, cur[b]])
        win[cur[active]] = B
        for b in active:  # ascending: the lowest blob that attains the key
            if p[b, cur[b]] == best[cur[b]] and win[cur[b]] == B:
                win[cur[b]] = b
        losers = [b for b in active if win[cur[b]] != b]
        passes += 1
        if not losers:
            break
        assert passes <= B, "more than B + 1 passes"
        for b in losers:
            at, atp = cur[b], p[b, cur[b]]
            row = p[b]
            behind = (row > 0.0) & ((row < atp) | ((row == atp) & (np.arange(L) > at)))
            can_win = (row > best) | ((row == best) & ~(win < b))
            cand = np.nonzero(behind & can_win)[0]
            cur[b] = cand[np.argmax(row[cand])] if cand.size else -1  # (argmax: the first of equal keys, landmarks ascend)
    return (cur + 1).astype(np.int32), passes


def min_competing_gap(prob):
    """The smallest relative difference between two positive probabilities of one row or one column of prob (inf: none compete):
    what has to stay clear of rounding for the device to order every blob's and every landmark's candidates as the oracle does."""
    p = _clean(prob)
    gap = np.inf
    for m in (p, p.T):
        s = np.sort(m, axis=1)
        hi, lo = s[:, 1:], s[:, :-1]
        both = lo > 0.0
        if both.any():
            gap = min(gap, float(((hi[both] - lo[both]) / hi[both]).min()))
    return gap


class UniqueAssociation(object):
    """Mixin in front of OracleFilter, BearingOracle or RangeBearingOracle: associate() settles the ids by the rule.  It keeps
    unique_stats  of the last association: particles whose maximum-likelihood ids claimed a landmark twice, blobs whose id changed,
                  of those the ones matched to another landmark, the most passes deferred_acceptance took
    unique_gap    the smallest min_competing_gap over the particles with a conflict, over every association made (inf: none)
    unique_floor  the smallest positive probability of those particles (the device must not see it underflow)"""

    unique_stats = (0, 0, 0, 0)
    unique_gap = np.inf
    unique_floor = np.inf  # the smallest positive probability of a particle with a conflict, over every association made

    def match_matrix(self, blobs, ranges, variances, p0, p1):
        """p(b, l) of particles [p0, p1): (p1 - p0, B, L), by the oracle's own model."""
        B = len(blobs)
        sx, sy, sh = self.x[p0:p1, None], self.y[p0:p1, None], self.h[p0:p1, None]
        mean, cov = self.mean[p0:p1], self.cov[p0:p1]
        out = np.zeros((p1 - p0, B, self.L))
        for b in range(B):
            if isinstance(self, rb.RangeBearingOracle) and not np.isnan(ranges[b]):
                out[:, b] = rb.probability_of_match(sx, sy, sh, blobs[b], ranges[b], variances[b], self.Qt[0, 0], mean, cov)
            elif isinstance(self, bearing.BearingOracle):
                out[:, b] = bearing.probability_of_match(sx, sy, sh, blobs[b], mean, cov)
            else:
                out[:, b] = reference_probability(sx, sy, sh, blobs[b], mean, cov)
        return _clean(out)

    def associate(self, blobs, ranges=None, variances=None, chunk=16):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = blobs.shape[0]
        ids = np.zeros((self.P, B), dtype=np.int32)
        stats = [0, 0, 0, 1 if B else 0]
        if self.L == 0 or B == 0:
            self.unique_stats = tuple(stats)
            return ids
        rng, var = rb._rows(B, ranges, variances)
        for p0 in range(0, self.P, chunk):
            p1 = min(self.P, p0 + chunk)
            pr = self.match_matrix(blobs, rng, var, p0, p1)
            for i in range(p1 - p0):
                ml = ml_ids(pr[i])
                claimed = ml[ml > 0]
                if len(np.unique(claimed)) == len(claimed):
                    ids[p0 + i] = ml
                    continue
                got = unique_ids(pr[i])
                da, passes = deferred_acceptance(pr[i])
                assert np.array_equal(got, da)
                self.unique_gap = min(self.unique_gap, min_competing_gap(pr[i]))
                self.unique_floor = min(self.unique_floor, float(pr[i][pr[i] > 0.0].min()))
                ids[p0 + i] = got
                stats[0] += 1
                stats[1] += int((got != ml).sum())
                stats[2] += int(((got != ml) & (got != 0)).sum())
                stats[3] = max(stats[3], passes)
        self.unique_stats = tuple(stats)
        return ids


# ---------------------------------------------------------------------------------------------------------------- the demonstration
# A small growing world under the bearing model: five preset landmarks of distinct colours and one UNKNOWN landmark (the twin) that
# has preset landmark 0's colour and stands 2 m beside it -- both inside one bearing gate for the whole drive.
TWIN_KNOWN = np.array([[12.0, 1.0, 200.0, 60.0, 40.0],
                       [9.0, 9.0, 30.0, 220.0, 60.0],
                       [15.0, -7.0, 40.0, 50.0, 230.0],
                       [4.0, -10.0, 230.0, 220.0, 30.0],
                       [18.0, 6.0, 120.0, 20.0, 160.0]])
TWIN_UNKNOWN = np.array([12.0, -1.0, 200.0, 60.0, 40.0])
TWIN_DRIVE = dict(v=0.6, w=0.04, dt=0.5, steps=40, sigma_bearing=0.004, sigma_colour=0.3, particles=16, spare=3, pair_threshold=30.0)


def twin_scene_run(association, seed, on_step=None):
    """The drive on the CPU oracle with association 'ml' or 'unique' -> the figures of the demonstration (a dict).  The same seed
    gives both modes the same noise.  on_step(step, oracle, blobs, z, u, ids): called behind every step (the GPU test follows it)."""
    from oracle.fastslam_oracle import low_variance_ancestors, truth_step

    d = TWIN_DRIVE
    P, L0 = d["particles"], len(TWIN_KNOWN)
    kcov = np.broadcast_to(0.25 * np.identity(5), (L0, 5, 5)).copy()
    o = bearing.under_bearing_model(GrowingOracle(P, TWIN_KNOWN, kcov, d["spare"], d["pair_threshold"]))
    if association == "unique":
        uniquely(o)
    world = np.vstack([TWIN_KNOWN, TWIN_UNKNOWN])
    rs = np.random.RandomState(seed)
    pose = (0.0, 0.0, 0.0)
    promoted_at = None
    for s in range(d["steps"]):
        pose = truth_step(pose, d["v"], d["w"], d["dt"])
        blobs = bearing.wrapped_scan(world, pose, rs, d["sigma_bearing"], d["sigma_colour"])
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        o.f.reset_weights()
        o.f.motion(d["v"], d["w"], d["dt"], z)
        ids = o.observe(blobs)
        if on_step:
            on_step(s, o, blobs, z, u, ids)
        o.gather(low_variance_ancestors(np.exp(o.f.logw - np.max(o.f.logw)), u))
        confirmed = (np.asarray(o.used) >= 1) & ~o.f.potential[:, L0] & (o.f.count[:, L0] > 5)
        if promoted_at is None and confirmed.all():
            promoted_at = s
    found = np.asarray(o.used) >= 1
    dist = np.hypot(o.f.mean[found, L0, 0] - TWIN_UNKNOWN[0], o.f.mean[found, L0, 1] - TWIN_UNKNOWN[1])
    known_err = np.hypot(o.f.mean[:, 0, 0] - TWIN_KNOWN[0, 0], o.f.mean[:, 0, 1] - TWIN_KNOWN[0, 1])
    return dict(association=association, seed=int(seed), promoted_at_step=promoted_at,
                particles_with_the_twin=int(found.sum()),
                twin_distance_from_truth=float(dist.mean()) if found.any() else None,
                known_error=float(known_err.mean()), known_updates=float((o.f.count[:, 0] // 2).mean()),
                readings_stored=float(np.mean([len(h) for h in o.hyp])))


_classes = {}


def uniquely(o):
    """The oracle `o` (an OracleFilter of any model, or a growing oracle whose filter is one) with the rule switched in; returns o.
    (The mixin adds no state of its own at construction, so a live object's class is simply replaced.)"""
    target = o.f if isinstance(o, GrowingOracle) else o
    assert isinstance(target, OracleFilter) and not isinstance(target, UniqueAssociation)
    cls = type(target)
    if cls not in _classes:
        _classes[cls] = type("Unique" + cls.__name__, (UniqueAssociation, cls), {})
    target.__class__ = _classes[cls]
    return o

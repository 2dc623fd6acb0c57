"""The exact reference of a WHOLE SCAN as one particle sees it, and the scenes the observe routes are held to it on.

What cam_cb does per particle behind the association (prkt_core_v2.py:73-124), in mpmath at ekf_reference.MP_BITS on top of
ekf_reference.exact_update: the blobs assigned to a landmark are applied to it in scan order (:88), the state staying in mpf from
update to update; an immutable landmark is weighed and not changed; a potential one (:109-118) weighs LOG_NO_MATCH, is updated,
and loses the bit when its count passes 5; every unmatched blob weighs LOG_NO_MATCH (:94-95, :851-857); the particle's log-weight
is W = carried + sum of the updates' log-weights + n_unmatched LOG_NO_MATCH.  The ids are an INPUT (safe_ids below forms them
from the reference's model and asserts that rounding cannot turn one), and so is the expected bearing of every update, as in
ekf_reference (atan2's own error is held by its own test and would be amplified by 1 / |innovation| here).

Units as in ekf_reference: |got - exact| / (2^-53 scale).  The scale of a field behind a chain of updates is the largest of the
chain's per-update scales, entry by entry (an error made by one update is carried through the later ones by I - K H, which does
not enlarge it); the scale of W is S = |carried| + sum max(logw_scale_i, 1) + n_unmatched |log 0.1| -- the max(., 1) pays for the
kernels that take one logarithm for several updates, whose error is absolute.

The bounds:
  a field behind a chain of n updates     units <= C_CHAIN n (32 + kappa_max^2 / 8)      kappa = cond_2(C + Qc), as ekf_reference
  W, a sum of T terms                     units <= (T - 1) + the largest field bound of the particle's chains
  the dense route, all 30 fields          units <= C_DENSE n (32 + kappa_q^2 / 8)        kappa_q = cond_2 of the whole 4x4 Q
The second is derived: any order of summing T terms costs at most (T - 1) 2^-53 sum |terms|, and each term is within its own
bound.  The constants are the smallest of 1, 2, 4, 8 at which the float64 oracle (OracleFilter.observe on the same ids) stays at or
below 0.6 of the bound on every scene they are for; tests/test_scan_reference_host.py measures them on the CPU and asserts the choice:

  C_CHAIN = 1, every class but the three below: the oracle's worst field is ORACLE_WORST_FIELD_RATIO of its bound (carried,
  L = 513), its worst W ORACLE_WORST_W_RATIO (general_qt, L = 40) -- 1 is the smallest on offer.
  C_EXTRA = 4, the classes EXTRA_CLASSES only (scaled_qt_m3, scaled_qt_m2, map_scale_large: chains at the last scales at which a
  float64 state still holds one, see scene()): the oracle's worst field is ORACLE_WORST_EXTRA_FIELD_RATIO (map_scale_large), its
  worst W ORACLE_WORST_EXTRA_W_RATIO (scaled_qt_m3); at 2 both are above 0.6.  These classes are beside the ones the routes are
  to be held on, not in their place, and their constant loosens no other class's bound.

Never set from what a device gives."""
import functools
import math

import numpy as np

import ekf_reference as er
from ekf_reference import COV_AT, LOG_NO_MATCH, POTENTIAL, units  # noqa: F401
from oracle import fastslam_oracle as O
from test_gpu_pub import poses_around

mpmath = er.mpmath
if mpmath is not None:
    from mpmath import mp, mpf

C_CHAIN = 1.0                      # measured on the CPU: at 1 the float64 oracle's worst over the scenes but EXTRA_CLASSES' is
ORACLE_WORST_FIELD_RATIO = 0.226   # ... of the bound of a field (carried, L = 513)
ORACLE_WORST_W_RATIO = 0.477       # ... of the bound of W (general_qt, L = 40)
EXTRA_CLASSES = ("scaled_qt_m3", "scaled_qt_m2", "map_scale_large")
C_EXTRA = 4.0                      # those classes' own constant, chosen the same way on them alone: at 4 the oracle's worst is
ORACLE_WORST_EXTRA_FIELD_RATIO = 0.407   # ... of the bound of a field (map_scale_large; at 2 it is 0.81)
ORACLE_WORST_EXTRA_W_RATIO = 0.524       # ... of the bound of W (scaled_qt_m3; at 2 it is 1.00)
C_DENSE = 1.0                      # the dense route's constant, chosen the same way on the dense scenes: the oracle's worst is
ORACLE_WORST_DENSE_FIELD_RATIO = 0.394   # ... of the bound of a field (typical, L = 9)
ORACLE_WORST_DENSE_W_RATIO = 0.300       # ... of the bound of W
PARTICLES = 3
SPREAD = 0.02
SIZES = (40, 512, 513, 1030, 2049, 3000)
MARGIN = 1e-6


def chain_constant(name):
    """the constant of a scene class's bounds: C_EXTRA for EXTRA_CLASSES, C_CHAIN for every other"""
    return C_EXTRA if name in EXTRA_CLASSES else C_CHAIN


def chain_bound(n, kappa, c=None):
    return (C_CHAIN if c is None else c) * n * er.update_bound(kappa)


# -------------------------------------------------------------------------------------------------------------- the exact scan
def exact_scan(pose, means, covs, counts, immutable, Qt, blobs, ids, zhat0, carried):
    """pose (P, 3+), means (L, 5) or (P, L, 5), covs (L, 5, 5) or (P, L, 5, 5), counts (L,) or (P, L) with the potential bit,
    immutable (L,) or None, Qt (4, 4), blobs (B, 4), ids (P, B) (0: unmatched), zhat0 (P, B) (NaN: atan2 of the exact state),
    carried (P,) or None.  -> one dict per particle:
      landmarks  {l: dict(mean 5 mpf, cov 5x5 mpf, mean_scale 5, cov_scale 5x5, count, n, kappa, kappa_q)} of the landmarks sighted
      W (mpf), S, T, n_unmatched (the bound of W: w_bound)."""
    er._ctx()
    pose = np.asarray(pose, dtype=np.float64)
    means, covs, counts = np.asarray(means, dtype=np.float64), np.asarray(covs, dtype=np.float64), np.asarray(counts)
    blobs, ids = np.asarray(blobs, dtype=np.float64).reshape(-1, 4), np.asarray(ids)
    P, B = ids.shape
    Qt_l = np.asarray(Qt, dtype=np.float64).tolist()
    log_no_match = mp.log(mpf(O.NO_MATCH_WEIGHT))  # the factor is the double 0.1 (:857)
    out = []
    for p in range(P):
        mp_, cp_, kp_ = (means[p], covs[p], counts[p]) if means.ndim == 3 else (means, covs, counts)
        sx, sy = float(pose[p, 0]), float(pose[p, 1])
        W = mpf(0.0 if carried is None else float(carried[p]))
        S = float(abs(W))
        lms, n_unmatched = {}, 0
        for b in range(B):
            l = int(ids[p, b]) - 1
            if l < 0:
                n_unmatched += 1
                W += log_no_match
                S += float(abs(log_no_match))
                continue
            st = lms.get(l)
            if st is None:
                st = lms[l] = dict(mean=[mpf(float(v)) for v in mp_[l]], cov=er._mat(cp_[l].tolist()), count=int(kp_[l]), n=0, kappa=0.0,
                                   kappa_q=0.0, mean_scale=[abs(float(v)) for v in mp_[l]], cov_scale=np.abs(cp_[l]).tolist())
            z0 = float(zhat0[p][b]) if zhat0 is not None else math.nan
            z0 = mp.atan2(st["mean"][1] - sy, st["mean"][0] - sx) if math.isnan(z0) else mpf(z0)  # :871
            row = [None] * 31
            row[er.E_SX], row[er.E_SY], row[er.E_ZHAT0] = sx, sy, z0
            row[er.E_F:er.E_F + 5] = st["mean"]
            row[er.E_BLOB:er.E_BLOB + 4] = [float(v) for v in blobs[b]]
            ex = er.exact_update(row, cov=st["cov"], Qt=Qt_l)
            if st["count"] & POTENTIAL:  # :111-112
                W += log_no_match
                S += float(abs(log_no_match))
            else:  # :121
                W += ex["logw"]
                S += max(ex["logw_scale"], 1.0)
            st["n"] += 1
            st["kappa"], st["kappa_q"] = max(st["kappa"], ex["kappa"]), max(st["kappa_q"], ex["kappa_q"])
            if immutable is None or not immutable[l]:
                st["mean"], st["cov"] = ex["mean"], ex["cov"]
                st["mean_scale"] = [max(a, c) for a, c in zip(st["mean_scale"], ex["mean_scale"])]
                st["cov_scale"] = [[max(a, c) for a, c in zip(r, s)] for r, s in zip(st["cov_scale"], ex["cov_scale"])]
                k = st["count"] + 2  # :914 and :930
                if (k & POTENTIAL) and (k & ~POTENTIAL) > 5:  # :113-117
                    k &= ~POTENTIAL
                st["count"] = k
        T = B + (1 if carried is not None else 0)  # terms of W
        out.append(dict(landmarks=lms, W=W, S=S, T=T, n_unmatched=n_unmatched))
    return out


def w_bound(e, c=None):
    """the bound of one particle's W, in units: (T - 1) + the largest field bound of its chains (c: the class's constant)"""
    return (e["T"] - 1) + max([chain_bound(st["n"], st["kappa"], c) for st in e["landmarks"].values()] + [0.0])


def compact_units(mean, cov, st):
    """worst units over the 14 compact fields of one landmark (mean (5,), cov (5, 5) as downloaded) against exact_scan's"""
    er._ctx()
    u = [units(mean[i], st["mean"][i], st["mean_scale"][i]) for i in range(5)]
    u += [max(units(cov[i, j], st["cov"][i][j], st["cov_scale"][i][j]), units(cov[j, i], st["cov"][j][i], st["cov_scale"][j][i])) for i, j in COV_AT]
    return max(u)


def dense_units(mean, cov, st):
    """worst units over the 30 fields of the dense layout: the 5 means and ALL 25 entries of the stored covariance, each against the
    exact entry in its place -- the exact Sigma' is symmetric, so the asymmetry of the stored one is held to the units of its entries"""
    er._ctx()
    u = [units(mean[i], st["mean"][i], st["mean_scale"][i]) for i in range(5)]
    u += [units(cov[i, j], st["cov"][i][j], st["cov_scale"][i][j]) for i in range(5) for j in range(5)]
    return max(u)


def dense_bound(n, kappa_q):
    return C_DENSE * n * er.update_bound(kappa_q)


def w_bound_dense(e):
    return (e["T"] - 1) + max([dense_bound(st["n"], st["kappa_q"]) for st in e["landmarks"].values()] + [0.0])


def scan_figures(ex, logw, means, covs, counts, dense=False, c=None):
    """One route's (or the oracle's) answer against exact_scan's ex: logw (P,), means (P, L, 5), covs (P, L, 5, 5), counts (P, L) ->
    dict(field_units, field_ratio, w_units, w_ratio, counts_equal), the worst over particles and landmarks.  dense: the 30 fields of
    the dense layout and the bounds in kappa_q = cond_2 of the whole Q.  c: the constant of the scene's class (chain_constant), C_CHAIN
    where none is given."""
    fig = dict(field_units=0.0, field_ratio=0.0, w_units=0.0, w_ratio=0.0, counts_equal=True)
    for p, e in enumerate(ex):
        for l, st in e["landmarks"].items():
            u = dense_units(means[p, l], covs[p, l], st) if dense else compact_units(means[p, l], covs[p, l], st)
            b = dense_bound(st["n"], st["kappa_q"]) if dense else chain_bound(st["n"], st["kappa"], c)
            fig["field_units"], fig["field_ratio"] = max(fig["field_units"], u), max(fig["field_ratio"], u / b)
            fig["counts_equal"] &= int(counts[p, l]) == st["count"]
        u = units(logw[p], e["W"], e["S"])
        fig["w_units"], fig["w_ratio"] = max(fig["w_units"], u), max(fig["w_ratio"], u / (w_bound_dense(e) if dense else w_bound(e, c)))
    return fig


# ------------------------------------------------------------------------------------------------------- the ids, and their safety
def log_probability(x, y, blob, mean, cov):
    """log of probability_of_match's product of the two densities (:439-455), without its gates and without underflow: float64"""
    nx, ny = O.closest_point(mean[..., 0], mean[..., 1], x, y, blob[0])
    ex, ey = nx - mean[..., 0], ny - mean[..., 1]
    sxx, sxy, syy = cov[..., 0, 0], cov[..., 0, 1], cov[..., 1, 1]
    det2 = sxx * syy - sxy * sxy
    with np.errstate(all="ignore"):
        maha2 = (syy * ex * ex - 2.0 * sxy * ex * ey + sxx * ey * ey) / det2
        (i00, i01, i02, i11, i12, i22), det3 = O.sym3_inv_det(cov[..., 2, 2], cov[..., 2, 3], cov[..., 2, 4], cov[..., 3, 3], cov[..., 3, 4], cov[..., 4, 4])
        d0, d1, d2 = blob[1] - mean[..., 2], blob[2] - mean[..., 3], blob[3] - mean[..., 4]
        maha3 = i00 * d0 * d0 + i11 * d1 * d1 + i22 * d2 * d2 + 2.0 * (i01 * d0 * d1 + i02 * d0 * d2 + i12 * d1 * d2)
        return -0.5 * (5.0 * math.log(O.TWO_PI) + np.log(det2) + np.log(det3) + maha2 + maha3)


def safe_ids(pose, means, covs, blobs, what=""):
    """The maximum-likelihood ids of the REFERENCE model (OracleFilter.associate's probabilities: the bearing difference not wrapped,
    :415) for particles at pose (P, 3+) that share one map, with the scene's safety asserted from the reference alone:
    no gate (:433, :441, :473-475) within 1e-6 of turning -- a gate's margin counts for the pairs the other gate does not itself
    reject by more than that margin, as in tests/test_gpu_proposal.py -- no two candidates of a blob within 1e-6 relative of each
    other, and no blob whose best candidate's probability is near the underflow of a double (between exp(-900) and 1e-250: a
    kernel and the reference could differ about it being positive, that is about the blob being matched at all).  -> (ids (P, B), passers (P, L): blobs inside both gates)."""
    pose, blobs = np.asarray(pose, dtype=np.float64), np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
    P, B, L = pose.shape[0], blobs.shape[0], means.shape[0]
    x, y, h = pose[:, 0:1], pose[:, 1:2], pose[:, 2:3]
    mean, cov = np.broadcast_to(means, (P, L, 5)), np.broadcast_to(covs, (P, L, 5, 5))
    pse = np.arctan2(mean[..., 1] - y, mean[..., 0] - x)
    expected = pse - h  # :408
    ids, passers = np.zeros((P, B), dtype=np.int32), np.zeros((P, L), dtype=np.int64)
    rows = np.arange(P)
    for b in range(B):
        delb = np.abs(blobs[b, 0] - expected)  # :415, not wrapped
        cd = np.power(blobs[b, 1] - mean[..., 2], 2) + np.power(blobs[b, 2] - mean[..., 3], 2) + np.power(blobs[b, 3] - mean[..., 4], 2)
        mb, mc = np.abs(delb - O.BEARING_GATE), np.abs(cd - O.COLOR_GATE)
        colour_rejects, bearing_rejects = (cd > O.COLOR_GATE) & (mc > MARGIN), (delb > O.BEARING_GATE) & (mb > MARGIN)
        close = ((mb <= MARGIN) & ~colour_rejects) | ((mc <= MARGIN) & ~bearing_rejects)
        assert not close.any(), (what, b, "a gate within 1e-6 of turning")
        inside = (delb <= O.BEARING_GATE) & (cd <= O.COLOR_GATE)
        side = np.abs(pse - blobs[b, 0])
        assert not (inside & (np.abs(side - math.pi / 2) <= MARGIN)).any(), (what, b, "the side gate within 1e-6 of turning")
        passers += inside
        pr = O.probability_of_match(x, y, h, blobs[b], mean, cov)
        pr = np.where(np.isnan(pr), 0.0, pr)
        assert not (pr[~inside] != 0.0).any()
        lp = np.where(inside & (side <= math.pi / 2), log_probability(x, y, blobs[b], mean, cov), -np.inf).max(axis=1)
        assert not ((lp < math.log(1e-250)) & (lp > -900.0)).any(), (what, b, "the best probability near the underflow")
        assert np.isfinite(pr).all(), (what, b)
        best = np.argmax(pr, axis=1)
        top = pr[rows, best]
        rest = pr.copy()
        rest[rows, best] = -1.0
        second = rest.max(axis=1) if L > 1 else np.zeros(P)
        assert not ((second > 0) & (top - second <= MARGIN * top)).any(), (what, b, "a tie between two candidates")
        ids[:, b] = np.where(top > 0.0, best + 1, 0)
    return ids, passers


# ------------------------------------------------------------------------------------------------------------------ the scenes
CLASSES = ("typical", "chains", "flags", "carried", "carried_fresh", "general_qt", "scaled_qt_m12", "scaled_qt_m6", "scaled_qt_m3", "scaled_qt_m2",
           "scaled_qt_p6", "scaled_qt_p12", "map_scale_small", "map_scale_large", "map_scale_huge", "norm_overflow", "norm_underflow")
SINGLES = ("scaled_qt_m12", "scaled_qt_m6")  # on the layout without second sightings, see scene()
MAP_SCALE_HUGE = 1e4
MAP_SCALE_SMALL = 1e-4  # (1e-6 cannot be made safe, see scene())
MAP_SCALE_LARGE = 1e3   # (with second sightings; at 1e4 the float64 oracle itself is at 140 times the bound there, see scene())


def _sightings(name, L, rs, longest):
    """[(landmark, sightings)] and the number of strays of a layout; the pair 2k, 2k + 1 first where the layout has one"""
    if name in ("typical", "singles"):
        n = min(40, L // 2)
        pick = rs.choice(L, n, replace=False)
        return [(int(l), 2 if i < 2 and name == "typical" else 1) for i, l in enumerate(pick)], 3
    if name == "flags":
        pick = rs.choice(L, 9 + 3 + 4, replace=False)
        return [(int(l), 1 + i % 3) for i, l in enumerate(pick[:9])] + [(int(pick[9]), 1), (int(pick[10]), 2), (int(pick[11]), 1)] + \
            [(int(l), 1) for l in pick[12:]], 2
    k = 2 * int(rs.randint(0, L // 2))
    rest = [int(l) for l in rs.permutation(L) if l not in (k, k + 1)]
    out = [(k, 4), (k + 1, 4), (rest[0], 2), (rest[1], 3), (rest[2], 4)] + [(l, 1) for l in rest[3:11]]
    if longest:
        out.append((rest[11], longest))
    return out, 2


@functools.lru_cache(maxsize=None)
def scene(name, L, longest=0):
    """One scene of a class on synthetic_world(L), from a fixed seed (the first of the seeds 7000 + ... whose draw meets the
    conditions: safe_ids passes; no landmark lets more than four blobs (or `longest`) through its gates; with chains and flags, every
    sighting is assigned to its landmark by every particle and a sighted landmark lets exactly its sightings through -- a draw that
    does not is a bad scene and is redrawn, no tolerance is widened for it).  PARTICLES particles in a cloud of spread 0.02 round the origin.  longest: one more landmark with that many
    sightings (5 .. 8 for the eight-slot sweep, 9 .. 12 for the general kernels).

      typical            Qt = 0.1 I; min(40, L / 2) landmarks sighted once, two of them twice, 3 strays
      chains             landmarks with 2, 3 and 4 sightings, the pair 2k, 2k + 1 with 4 each, 8 with one, 2 strays
      flags              potential landmarks with counts 0 .. 8 and 1, 2, 3 sightings (some promoted in mid-chain), three immutable
                         ones (one of them potential, one with two sightings), four plain ones
      carried(_fresh)    typical, behind uploaded log-weights of -1e4 u (fresh: the same scan with the weights restarted)
      general_qt         chains; Qt's colour block symmetric positive definite with off-diagonal terms, as ekf_reference's class
      scaled_qt_*        Qt = 0.1 I x 10^k.  k = +6, +12, -2, -3 on chains, a landmark's later sightings drawn with 10^(k/2) times the
                         noise where k < 0.  k = -6 and -12 on the layout of typical WITHOUT second sightings (40 landmarks sighted
                         once, 3 strays): a chain there cannot be held by ANY float64 state -- behind the first update the colour
                         mean sits on the blob, rounded to a double (an ulp of 255 is 2.8e-14), and the next innovation is
                         measured in sqrt(Qt), so the Mahalanobis term is off by 2 (d / sigma) (ulp / sigma); measured on the
                         float64 oracle, W of the chains scene is at 2 800 times the bound at k = -6, 40 times at k = -4, inside
                         it at k = -3 (tests/test_scan_reference_host.py measures the classes here on every run)
      map_scale_*        the covariance blocks x 1e-4 (small) and x 1e3 (large) on typical, x 1e4 (huge) on the layout without
                         second sightings; the blobs' noise in proportion, capped by the gates (0.1 rad, 4 colour units).  1e-6
                         cannot be made safe: a position block of 2.5e-7 is 5e-4 m wide and the cloud 0.02, so for some particles
                         the position density of the RIGHT landmark is exp(-800), below the doubles; 1e-4 is the nearest power of
                         100 that is safe.  At x 1e4 a second sighting puts the float64 oracle itself at 140 times the bound of W
                         (measured), a single one leaves it at 0.04; 1e3 is the largest scale at which it holds a chain.
                         scaled_qt_m2, scaled_qt_m3 and map_scale_large are EXTRA_CLASSES: beside the scales asked for, with
                         a constant of their own (C_EXTRA), which no other class's bound sees.
      norm_overflow      chains; the colour block of Qt 1e20 I: every update has fro2 = 3e40.  NOT built: a lane whose first
                         pair has 3 sightings and whose second has 5 (L >= 1030).  The publishing kernels rank a scan's octets
                         of landmarks by cost and deal them out so that two octets share a lane only at ranks 64 apart
                         (k_step_pub<2, 512>: g >> 3 against g & 7; k_step_pub_big: s_bperm[64 q + (t >> 3)]); an octet with
                         a sighted landmark costs at least one pass, so a lane with two sighted pairs needs 64 octets of at
                         least that cost, which at most 48 blobs cannot sight.  Nor do the kernels have code at the pair
                         boundary any more: the product is tested behind every factor, and the probe test
                         (tests/test_gpu_ekf_reference.py::test_the_product_of_norms_never_leaves_the_normal_numbers) feeds
                         ekf_update a product of 3e40^7 and the eighth factor.
      norm_underflow     chains; all particles at one pose, every landmark immutable with P = C = 1e-20 I, Qt = 1e-20 I, the blobs'
                         colours the means and their bearings atan2 from that pose: fro2 = 1.3e-39"""
    base = {"general_qt": "chains", "norm_overflow": "chains", "norm_underflow": "chains"}.get(name, "chains" if name.startswith("scaled_qt") else name)
    base = "typical" if base.startswith("map_scale") or base.startswith("carried") else base
    if name in SINGLES or name == "map_scale_huge" or name.endswith("_singles"):
        base = "singles"
    last = None
    for attempt in range(40):
        rs = np.random.RandomState(7000 + 100 * (CLASSES.index(name) if name in CLASSES else 50 + sum(map(ord, name))) + attempt)
        try:
            return _draw(name, base, L, longest, rs)
        except AssertionError as e:
            last = e
    raise AssertionError("no safe draw of %s at L = %d: %r" % (name, L, last))


def _draw(name, base, L, longest, rs):
    means, covs = O.synthetic_world(L)
    pose = poses_around(rs, PARTICLES, SPREAD)
    sight, strays = _sightings(base, L, rs, longest)
    Qt = 0.1 * np.identity(4)
    counts = np.zeros(L, dtype=np.int32)
    immutable, carried, fresh = None, None, True
    sb, sc, later = 0.01, 0.4, 1.0  # the blobs' noise: bearing (rad), colour (a channel); a landmark's later sightings: x later
    if name.startswith("map_scale"):
        k = {"small": MAP_SCALE_SMALL, "large": MAP_SCALE_LARGE, "huge": MAP_SCALE_HUGE}.get(name.split("_")[2]) or float(name.split("_")[2])
        covs, sb, sc = covs * k, min(sb * math.sqrt(k), 0.1), min(sc * math.sqrt(k), 4.0)
    elif name == "general_qt":
        Qt = np.zeros((4, 4))
        Qt[0, 0] = rs.uniform(0.02, 0.5)
        q = er._spd3(rs, er._lam3(rs, rs.uniform(0.05, 0.5, 1), er._log_uniform(rs, 2.0, 8.0, 1)))[0]
        Qt[1:, 1:] = er.dense_qt(np.concatenate([[0.0], q]))[1:, 1:]
    elif name.startswith("scaled_qt"):
        k = int(name.split("_")[-1][1:]) * (-1 if name.split("_")[-1][0] == "m" else 1)
        Qt = Qt * 10.0 ** k
        later = min(1.0, 10.0 ** (k / 2.0))
    elif name == "norm_overflow":
        Qt[1:, 1:] = 1e20 * np.identity(3)
    elif name == "norm_underflow":
        pose[:, :3] = pose[0, :3]
        pose[:, 2] = 0.0
        covs = np.broadcast_to(1e-20 * np.identity(5), (L, 5, 5)).copy()
        Qt = 1e-20 * np.identity(4)
        immutable = np.ones(L, dtype=bool)
        sb = sc = 0.0
    elif name == "flags":
        immutable = np.zeros(L, dtype=bool)
        for i, (l, _) in enumerate(sight):
            if i < 9:
                counts[l] = i | POTENTIAL
            elif i < 12:
                immutable[l] = True
                counts[l] = (3 | POTENTIAL) if i == 9 else 4
            else:
                counts[l] = int(rs.randint(0, 9))
    elif name == "carried":
        carried, fresh = -1e4 * rs.uniform(0.0, 1.0, PARTICLES), False
    elif name == "carried_fresh":
        carried = -1e4 * rs.uniform(0.0, 1.0, PARTICLES)
    origin = pose[0, :2] if name == "norm_underflow" else np.zeros(2)
    owner = np.array([l + 1 for l, n in sight for _ in range(n)] + [0] * strays, dtype=np.int32)[rs.permutation(sum(n for _, n in sight) + strays)]
    blobs, seen = [], set()
    for own in owner:  # in scan order: a landmark's later sightings are drawn with `later` times the noise of its first
        if own == 0:
            for _ in range(400):
                z = np.concatenate([[rs.uniform(-3.0, 3.0)], rs.uniform(0.0, 255.0, 3)])
                if not safe_ids(pose, means, covs, z[None, :])[1].any():
                    break
            else:
                raise AssertionError("no stray")
        else:
            l, k = own - 1, (later if own in seen else 1.0)
            seen.add(own)
            bearing = np.arctan2(means[l, 1] - origin[1], means[l, 0] - origin[0]) + k * sb * rs.standard_normal()
            z = np.concatenate([[bearing], means[l, 2:] + k * sc * rs.standard_normal(3)])
        blobs.append(z)
    blobs = np.array(blobs)
    ids, passers = safe_ids(pose, means, covs, blobs, what=(name, L))
    want = np.zeros(L, dtype=np.int64)
    for l, n in sight:
        want[l] = n
    if base in ("chains", "flags"):  # the chains are the ones stated
        assert np.array_equal(ids, np.broadcast_to(owner, ids.shape)), "a sighting that is not assigned to its landmark"
        assert np.array_equal(passers[:, want > 0], np.broadcast_to(want[want > 0], (PARTICLES, int((want > 0).sum())))), "other blobs inside a sighted landmark's gates"
    assert passers.max() <= max(4, longest), "more blobs inside a landmark's gates than the route keeps"
    assert len(blobs) <= 48
    s = dict(name=name, L=L, longest=longest, pose=np.concatenate([pose[:, :3], np.ones((PARTICLES, 1))], axis=1), means=means, covs=covs, counts=counts,
             immutable=immutable, Qt=Qt, blobs=blobs, ids=ids, carried=carried, fresh=fresh, sight=tuple(sight), most=int(passers.max()),
             pair=(sight[0][0], sight[1][0]) if base == "chains" else None)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


# -------------------------------------------------------------------------------------------------- the dense route's scenes
DENSE_CLASSES = ("typical", "chains", "flags", "carried", "cond_q")
DENSE_SIZES = (9, 60)


@functools.lru_cache(maxsize=None)
def dense_scene(name, L):
    """The dense route (k_observe_dense): landmark covariances that couple position and colour and a Qt that couples bearing and
    colour (dense_world and random_spd of tests/test_gpu_dense.py), L in {9, 60}; the same conditions on a draw as scene().
      typical   min(40, L) landmarks sighted once, two of them twice, 3 strays
      chains    landmarks with 2, 3 and 4 sightings, a pair 2k, 2k + 1 with 4 each, the rest (up to 8) once, 2 strays
      flags     potential landmarks with counts 0, 2, 4, 5, 8 and 1, 2, 3 sightings, two immutable ones, the rest (up to 4) plain
      carried   typical behind uploaded log-weights of -1e4 u
      cond_q    landmarks sighted once; Qt 1e-6 of the usual, the covariances' eigenvalues spread so that cond_2(Q) is
                log-uniform up to 1e5 (the host test asserts the range reached)"""
    last = None
    for attempt in range(40):
        rs = np.random.RandomState(8000 + 100 * DENSE_CLASSES.index(name) + L + 1000 * attempt)
        try:
            return _draw_dense(name, L, rs)
        except AssertionError as e:
            last = e
    raise AssertionError("no safe draw of the dense %s at L = %d: %r" % (name, L, last))


def _draw_dense(name, L, rs):
    from test_gpu_dense import dense_world, random_spd

    _, means, covs, imm = dense_world(int(rs.randint(1, 1 << 30)), L)
    pose = poses_around(rs, PARTICLES, SPREAD)
    Qt = random_spd(rs, 4, 0.1)
    counts, immutable, carried, fresh, strays = np.zeros(L, dtype=np.int32), None, None, True, 3
    perm = [int(l) for l in rs.permutation(L)]
    if name in ("typical", "carried"):
        sight = [(l, 2 if i < 2 else 1) for i, l in enumerate(perm[:min(40, L)])]
        if name == "carried":
            carried, fresh = -1e4 * rs.uniform(0.0, 1.0, PARTICLES), False
    elif name == "chains":
        k = 2 * int(rs.randint(0, L // 2))
        rest = [l for l in perm if l not in (k, k + 1)]
        sight, strays = [(k, 4), (k + 1, 4), (rest[0], 2), (rest[1], 3), (rest[2], 4)] + [(l, 1) for l in rest[3:11]], 2
    elif name == "flags":
        sight, strays = [(l, 1 + i % 3) for i, l in enumerate(perm[:5])] + [(perm[5], 2), (perm[6], 1)] + [(l, 1) for l in perm[7:11]], 2
        immutable = np.zeros(L, dtype=bool)
        for i, c in enumerate((0, 2, 4, 5, 8)):
            counts[perm[i]] = c | POTENTIAL
        immutable[[perm[5], perm[6]]] = True
        counts[perm[6]] = 3 | POTENTIAL
    else:  # cond_q
        sight = [(l, 1) for l in perm[:min(40, L)]]
        Qt = 1e-6 * Qt
        for l in range(L):
            q, _ = np.linalg.qr(rs.normal(size=(5, 5)))
            lam = 0.5 * 10.0 ** -rs.uniform(0.0, 5.0) ** np.linspace(0.0, 1.0, 5)
            covs[l] = (q * lam) @ q.T
            covs[l] = 0.5 * (covs[l] + covs[l].T)
    owner = np.array([l + 1 for l, n in sight for _ in range(n)] + [0] * strays, dtype=np.int32)[rs.permutation(sum(n for _, n in sight) + strays)]
    blobs = []
    for own in owner:
        if own == 0:
            for _ in range(400):
                z = np.concatenate([[rs.uniform(-3.0, 3.0)], rs.uniform(0.0, 255.0, 3)])
                if not safe_ids(pose, means, covs, z[None, :])[1].any():
                    break
            else:
                raise AssertionError("no stray")
        else:
            l = own - 1
            z = np.concatenate([[np.arctan2(means[l, 1], means[l, 0]) + 0.01 * rs.standard_normal()], means[l, 2:] + 0.4 * rs.standard_normal(3)])
        blobs.append(z)
    blobs = np.array(blobs)
    ids, passers = safe_ids(pose, means, covs, blobs, what=("dense", name, L))
    assert np.array_equal(ids, np.broadcast_to(owner, ids.shape)), "a sighting that is not assigned to its landmark"
    assert len(blobs) <= 48
    s = dict(name=name, L=L, longest=0, pose=np.concatenate([pose[:, :3], np.ones((PARTICLES, 1))], axis=1), means=means, covs=covs, counts=counts,
             immutable=immutable, Qt=Qt, blobs=blobs, ids=ids, carried=carried, fresh=fresh, sight=tuple(sight), most=int(passers.max()), pair=None)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _exact_dense(name, L, zhat0_bytes):
    s = dense_scene(name, L)
    zhat0 = np.frombuffer(zhat0_bytes, dtype=np.float64).reshape(s["ids"].shape)
    return exact_scan(s["pose"], s["means"], s["covs"], s["counts"], s["immutable"], s["Qt"], s["blobs"], s["ids"], zhat0,
                      s["carried"] if not s["fresh"] else None)


def exact_dense(s, zhat0):
    return _exact_dense(s["name"], s["L"], np.ascontiguousarray(zhat0, dtype=np.float64).tobytes())


# ------------------------------------------------------------------------------------------ the float64 oracle on the same scene
def oracle_scan(s):
    """OracleFilter.observe on the scene with the scene's ids, blob by blob -> (logw (P,), means, covs, counts with the potential
    bit, atan_args (P, B, 2): dy, dx of the landmark a blob is applied to, from the state the blob meets)"""
    P, B = s["ids"].shape
    shared = np.ndim(s["means"]) == 2  # (one map for every particle, or each its own)
    o = O.OracleFilter(P, s["means"] if shared else s["means"][0], s["covs"] if shared else s["covs"][0], immutable=s["immutable"], Qt=s["Qt"])
    if not shared:
        o.mean, o.cov = np.array(s["means"], dtype=np.float64), np.array(s["covs"], dtype=np.float64)
    o.x, o.y, o.h = s["pose"][:, 0].copy(), s["pose"][:, 1].copy(), s["pose"][:, 2].copy()
    o.count[:] = s["counts"] & ~POTENTIAL
    o.potential[:] = (s["counts"] & POTENTIAL) != 0
    if s["carried"] is not None and not s["fresh"]:
        o.logw[:] = s["carried"]
    args = np.full((P, B, 2), np.nan)
    with np.errstate(all="ignore"):
        for b in range(B):
            for p in range(P):
                l = s["ids"][p, b] - 1
                if l >= 0:
                    args[p, b] = o.mean[p, l, 1] - o.y[p], o.mean[p, l, 0] - o.x[p]
            o.observe(s["blobs"][b:b + 1], ids=s["ids"][:, b:b + 1])
    counts = o.count.astype(np.int64) | np.where(o.potential, POTENTIAL, 0)
    return o.logw.copy(), o.mean, o.cov, counts, args


@functools.lru_cache(maxsize=None)
def _exact_scene(name, L, longest, zhat0_bytes):
    s = scene(name, L, longest)
    zhat0 = np.frombuffer(zhat0_bytes, dtype=np.float64).reshape(s["ids"].shape)
    return exact_scan(s["pose"], s["means"], s["covs"], s["counts"], s["immutable"], s["Qt"], s["blobs"], s["ids"], zhat0,
                      s["carried"] if not s["fresh"] else None)


def exact_scene(s, zhat0):
    """exact_scan of a scene with the expected bearings zhat0 (P, B): computed once per (scene, zhat0), shared, never changed"""
    return _exact_scene(s["name"], s["L"], s["longest"], np.ascontiguousarray(zhat0, dtype=np.float64).tobytes())


# ------------------------------------------------------------------------------------------------------------------ the routes
# per map size (each the smallest on its side of a routing boundary): name -> (options, observe_route(), observe_published());
# the kernels: ml_fused k_step_fused (published: k_step_pub<256>), ml_handoff the hand-off with k_observe_fast, ml_sweep
# k_observe_sweep (fast_observe = 3: eight slots), ml_general k_observe, ml_regs k_step_regs (published: k_step_pub, one pair a
# lane up to 1 024 landmarks, two beyond, where the lean groups are), ml_pub_big k_step_pub_big
ROUTES = {
    40: {"fused": ({}, "ml_fused", 0), "pub256": ({"pub_small": 1}, "ml_fused", 1), "general": ({"fast_observe": 0}, "ml_general", 0),
         "handoff": ({"fused_step": 0, "regs_step": 0}, "ml_handoff", 0), "sweep4": ({"fast_observe": 2}, "ml_sweep", 0),
         "sweep8": ({"fast_observe": 3}, "ml_sweep", 0)},
    512: {"fused": ({"pub_small": 0}, "ml_fused", 0), "pub256": ({"pub_small": 1}, "ml_fused", 1),
          "handoff": ({"fused_step": 0, "regs_step": 0}, "ml_handoff", 0)},
    513: {"pub": ({}, "ml_regs", 1), "pub_no_table": ({"colour_table": 0}, "ml_regs", 1), "sweep4": ({"fused_step": 0, "regs_step": 0}, "ml_sweep", 0),
          "sweep8": ({"fast_observe": 3}, "ml_sweep", 0)},
    1030: {"pub": ({}, "ml_regs", 1), "pub_no_table": ({"colour_table": 0}, "ml_regs", 1), "pub_no_lean": ({"pub_lean": 0}, "ml_regs", 1),
           "regs": ({"pub_step": 0}, "ml_regs", 0), "general": ({"assoc_kernel": 1}, "ml_general", 0), "sweep4": ({"fast_observe": 2}, "ml_sweep", 0)},
    2049: {"pub_big": ({}, "ml_pub_big", 1), "sweep4": ({"pub_step": 0}, "ml_sweep", 0)},
    3000: {"pub_big": ({}, "ml_pub_big", 1), "sweep8": ({"fast_observe": 3}, "ml_sweep", 0), "general": ({"fast_observe": 0}, "ml_general", 0)},
}
PUBLISHING = ("pub256", "pub", "pub_no_table", "pub_no_lean", "pub_big")  # the instances that fold the norms of a lane's updates

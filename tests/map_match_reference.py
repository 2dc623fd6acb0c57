"""The reference of the discovered-landmark tests (pk_map_match_moments / pk_map_discovered): the matching rule in NumPy float64
with the device's operation order -- so the match table is EXACT -- and then a two-pass computation of every feature's moments
about its true mean over the matched slots, in the style of mapsum_reference.two_pass.  Shared by test_map_match_host.py and
test_gpu_map_discovered.py; so is the generator of planted states.

The rule.  Candidates of particle p: its spare slots 0 .. u_p - 1 (u_p = counter word 1, clamped to S), landmarks L0 + i.  With
dx = mu_x - r_x ...: dpos2 = dx dx + dy dy, dcol2 = (dr dr + dg dg) + db db; a candidate passes iff dpos2 <= rho rho and
dcol2 <= kappa kappa; score = dpos2 (1 / rho^2) + dcol2 (1 / kappa^2), the reciprocals 0 for an infinite radius; the match is the
passing candidate with the strictly smallest score, the lowest slot among equals (NumPy's elementwise products and sums are not
fused, like the device code under `fp contract(off)`).

Tolerances (mapsum_reference.check's, the project's own): a mean entry to 1e-12 of max(|entry|, its standard deviation in the
mixture); a covariance entry [i][j] -- total, within or between -- to 1e-10 of sqrt(c_ii c_jj), c the reference's TOTAL covariance;
support, potential_fraction, update_count and every n_eff to 1e-12 relative; the match table exact."""
import numpy as np

from mapsum_reference import POT, block_diagonal_covs


class Ref(object):
    pass


def match_table(means, used, L0, ref, radius, colour_radius):
    """means (P, L, 5), used (P,), ref (n, 5) -> matches (P, n) int32 (-1: none), passing (P, n) the number of candidates inside
    both gates, tie (P, n) True where the two smallest scores are equal."""
    means = np.asarray(means, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 5)
    P, L = means.shape[:2]
    S = L - L0
    u = np.clip(np.asarray(used).astype(np.int64), 0, S)
    rho2 = np.float64(radius) * np.float64(radius)
    kap2 = np.float64(colour_radius) * np.float64(colour_radius)
    irho2 = 0.0 if np.isinf(rho2) else 1.0 / rho2
    ikap2 = 0.0 if np.isinf(kap2) else 1.0 / kap2
    cand = means[:, L0:, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = [cand[:, None, :, k] - ref[None, :, None, k] for k in range(5)]  # (P, n, S) each
        dpos2 = d[0] * d[0] + d[1] * d[1]
        dcol2 = (d[2] * d[2] + d[3] * d[3]) + d[4] * d[4]
        ok = (dpos2 <= rho2) & (dcol2 <= kap2) & (np.arange(S)[None, None, :] < u[:, None, None])
        score = dpos2 * irho2 + dcol2 * ikap2
        key = np.where(ok & (score < np.inf), score, np.inf)  # (a score that is not below +inf never stands: the device's `<`)
    if S == 0:
        none = np.full((P, ref.shape[0]), -1, dtype=np.int32)
        return none, np.zeros(none.shape, dtype=np.int64), np.zeros(none.shape, dtype=bool)
    best = np.argmin(key, axis=2)  # the first of the smallest: the lowest slot among equals
    low = np.take_along_axis(key, best[:, :, None], axis=2)[:, :, 0]
    matches = np.where(low < np.inf, best, -1).astype(np.int32)
    two = np.sort(key, axis=2)[:, :, :2]
    tie = (two[:, :, 0] < np.inf) & (two[:, :, 0] == two[:, :, -1]) if S > 1 else np.zeros(matches.shape, dtype=bool)
    return matches, ok.sum(axis=2), tie


def reference(means, covs, counts, used, L0, ref, radius, colour_radius, w=None):
    """The finished estimate per reference feature over all particles: matches, then two passes per feature."""
    means = np.asarray(means, dtype=np.float64)
    P, L = means.shape[:2]
    covs = np.asarray(covs, dtype=np.float64).reshape(P, L, 5, 5)
    counts = np.asarray(counts).astype(np.int64).reshape(P, L)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 5)
    n = ref.shape[0]
    w = np.ones(P) if w is None else np.asarray(w, dtype=np.float64).reshape(P)
    r = Ref()
    r.matches, r.passing, r.tie = match_table(means, used, L0, ref, radius, colour_radius)
    r.W, r.W2 = w.sum(), (w * w).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        r.n_eff_all = r.W * r.W / r.W2
    r.Wj, r.support, r.potential_fraction, r.n_eff, r.count = (np.zeros(n) for _ in range(5))
    r.mean = np.full((n, 5), np.nan)
    r.m2 = np.full((n, 5, 5), np.nan)
    r.wsigma = np.zeros((n, 5, 5))
    r.wcount, r.W2j, r.Wpot = np.zeros(n), np.zeros(n), np.zeros(n)
    r.holders = (r.matches >= 0).sum(axis=0)
    for j in range(n):
        p = np.nonzero(r.matches[:, j] >= 0)[0]
        l = L0 + r.matches[p, j]
        wp, mu, c = w[p], means[p, l], counts[p, l]
        r.Wj[j], r.W2j[j] = wp.sum(), (wp * wp).sum()
        r.Wpot[j] = wp[(c & POT) != 0].sum()
        r.wsigma[j] = np.einsum("p,pij->ij", wp, covs[p, l])
        r.wcount[j] = (wp * (c & ~POT).astype(np.float64)).sum()
        if r.Wj[j] > 0.0:
            r.mean[j] = np.einsum("p,pi->i", wp, mu) / r.Wj[j]
            d = mu - r.mean[j]
            r.m2[j] = np.einsum("p,pi,pj->ij", wp, d, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        Wj = r.Wj[:, None, None]
        r.between = r.m2 / Wj
        r.within = r.wsigma / Wj
        r.cov = r.within + r.between
        r.count = r.wcount / r.Wj
        r.support = r.Wj / r.W
        r.potential_fraction = r.Wpot / r.Wj
        r.n_eff = r.Wj * r.Wj / r.W2j
    return r


def moments_of(r):
    """The reference as unfinished moments (parakeet_slam_amd.mapsum.MatchedMoments): what pk_map_match_moments hands out."""
    from mapsum_reference import TRI, WITHIN_IJ
    from parakeet_slam_amd import mapsum

    within = np.stack([r.wsigma[:, i, j] for i, j in WITHIN_IJ], axis=1)
    return mapsum.MatchedMoments([r.W, r.W2], np.stack([r.Wj, r.W2j, r.Wpot], axis=1), r.mean, r.m2[:, TRI[0], TRI[1]], within, r.wcount,
                                 r.matches)


def worst(got, ref):
    """The largest error of each kind over its tolerance (<= 1 passes), as a dict; got: mapsum.DiscoveredMap."""
    held = ref.Wj > 0.0
    out = {}
    for name in ("mean", "cov", "cov_within", "cov_between", "update_count", "potential_fraction", "n_eff"):
        a = getattr(got, name)
        assert np.isnan(a[~held]).all(), "%s: a feature nobody matched must be NaN" % name
        assert not np.isnan(a[held]).any(), "%s: NaN in a feature somebody matched" % name
    assert (got.support[~held] == 0.0).all(), "a feature nobody matched has support 0"
    sd = np.sqrt(np.einsum("lii->li", ref.cov[held]))
    out["mean"] = float(np.max(np.abs(got.mean[held] - ref.mean[held]) / (1e-12 * np.maximum(np.abs(ref.mean[held]), sd)), initial=0.0))
    scale = 1e-10 * sd[:, :, None] * sd[:, None, :]
    for name in ("cov", "within", "between"):
        g = getattr(got, "cov" if name == "cov" else "cov_" + name)[held]
        assert np.array_equal(g, np.swapaxes(g, 1, 2)), name + " is not symmetric"
        out[name] = float(np.max(np.abs(g - getattr(ref, name)[held]) / scale, initial=0.0))

    def rel(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if not np.array_equal(a[b == 0.0], b[b == 0.0]):  # (a sum of nothing, or of zeros, is exact)
            return np.inf
        nz = b != 0.0
        return float(np.max(np.abs(a[nz] - b[nz]) / (1e-12 * np.abs(b[nz])), initial=0.0))

    out["count"] = rel(got.update_count[held], ref.count[held])
    out["support"] = rel(got.support, ref.support)
    out["potential"] = rel(got.potential_fraction[held], ref.potential_fraction[held])
    out["n_eff"] = rel(got.n_eff[held], ref.n_eff[held])
    out["n_eff_all"] = abs(got.n_eff_all - ref.n_eff_all) / (1e-12 * ref.n_eff_all)
    return out


def check(got, ref, what=""):
    w = worst(got, ref)
    print("discovered landmarks %s: error / tolerance %s" % (what, {k: "%.3g" % v for k, v in w.items()}))
    assert all(v <= 1.0 for v in w.values()), (what, w)
    return w


# ---- planted states: a few "true" features, every particle holding a random subset of them in a random slot order, and decoys
RADIUS, COLOUR_RADIUS = 3.0, 30.0


def true_features(n, offset=0.0):
    """n features >= 10 apart in position (a grid) and >= 85 apart in colour (a lattice; colours are plain numbers here)."""
    k = np.arange(n)
    t = np.empty((n, 5))
    t[:, 0], t[:, 1] = offset + 10.0 * (k % 9), offset + 10.0 * (k // 9)
    t[:, 2], t[:, 3], t[:, 4] = 85.0 * (k % 5), 85.0 * ((k // 5) % 5), 85.0 * (k // 25)
    return t


def planted_state(P, L0, S, seed, offset=0.0, noise=0.01, assert_conditions=True):
    """A state for DeviceFilter(P, L0 + S): dict of means (P, L, 5), covs (P, L, 5, 5), counts (P, L) int32, used (P,), slot_ids
    (P, S), truth (S, 5), base (L, 5).  Every particle holds some of the S true features (position noise `noise` << RADIUS, colour
    noise 50 x that) in a random slot order, or decoys about a true feature t:
      colour  a slot at t + (1, 0) in the wrong colour (+100): inside the position gate, outside the colour gate
      outside a slot in the right colour at t + (RADIUS + 0.05, 0): just outside the position gate; the particle does not hold t
      two     t itself and a second slot in the right colour at t + (1.5, 0): both pass, the nearer wins
      tie     two slots at t -+ (0.5, 0), exactly, same y and colours, t itself not held: equal scores, the lower slot wins
    The slots beyond u_p hold exact copies of true features: they would match if they were read.  Particle 0 is a tie particle
    (S >= 2), particle 1 holds nothing, particle 2 all S features.  The generator asserts what it promises (against the explicit
    references `truth`): a tie when S >= 2; u_p covering 0 and S when P >= 3; and, for P >= 257 and S >= 6, at least 10 % of the
    (particle, feature) pairs unmatched and at least 5 % decided between two passing candidates."""
    rs = np.random.RandomState(seed)
    L = L0 + S
    t = true_features(S, offset)
    base = np.zeros((L, 5))
    base[:L0, 0], base[:L0, 1] = offset + 1000.0 + 10.0 * np.arange(L0), offset - 500.0
    base[:L0, 2:] = 40.0
    base[L0:, 2:] = 9999.0
    means = np.broadcast_to(base, (P, L, 5)).copy()
    means[:, :L0] += 0.3 * rs.standard_normal((P, L0, 5))
    used = np.zeros(P, dtype=np.int32)
    jitter = np.array([noise, noise, 50 * noise, 50 * noise, 50 * noise])
    for p in range(P):
        kind = rs.choice(["plain", "two", "colour", "outside", "tie"], p=[0.4, 0.3, 0.1, 0.1, 0.1])
        kind = {0: "tie", 1: "empty", 2: "full"}.get(p, kind)
        if S < 2 and kind != "empty":
            kind = "full" if p == 2 else "plain"
        order = rs.permutation(S)
        slots = []
        if kind == "full":
            slots = [t[k] + jitter * rs.standard_normal(5) for k in order]
        elif kind == "plain":
            slots = [t[k] + jitter * rs.standard_normal(5) for k in order[:rs.randint(0, S + 1)]]
        elif kind == "two":
            held = order[:max(S // 2, 1)]
            slots = [t[k] + jitter * rs.standard_normal(5) for k in held]
            slots += [t[k] + np.array([1.5, 0, 0, 0, 0]) + jitter * rs.standard_normal(5) for k in held[:S - len(held)]]
        elif kind in ("colour", "outside"):
            held = order[1:1 + rs.randint(0, S)]
            if kind == "colour" and rs.uniform() < 0.5:
                held = np.append(held, order[0])  # (with and without the true feature beside its decoy)
            slots = [t[k] + jitter * rs.standard_normal(5) for k in held[:S - 1]]
            shift = np.array([1.0, 0, 100.0, 0, 0]) if kind == "colour" else np.array([RADIUS + 0.05, 0, 0, 0, 0])
            slots.append(t[order[0]] + shift)
        elif kind == "tie":
            slots = [t[k] + jitter * rs.standard_normal(5) for k in order[1:S - 1]]
            slots += [t[order[0]] - np.array([0.5, 0, 0, 0, 0]), t[order[0]] + np.array([0.5, 0, 0, 0, 0])]
        u = len(slots)
        assert u <= S
        used[p] = u
        place = rs.permutation(u)
        for i, s in zip(place, slots):
            means[p, L0 + i] = s
        means[p, L0 + u:] = t[rs.randint(0, S, size=S - u)]  # not candidates: nobody may read them
    covs = block_diagonal_covs(rs, P, L)
    counts = rs.randint(0, 40, size=(P, L)).astype(np.int32)
    counts[:, L0:][rs.uniform(size=(P, S)) < 0.3] |= POT
    slot_ids = rs.randint(L0 + 1, L0 + 1000, size=(P, S)).astype(np.int32)
    st = dict(means=means, covs=covs, counts=counts, used=used, slot_ids=slot_ids, truth=t, base=base, P=P, L0=L0, S=S)
    if assert_conditions:
        m, passing, tie = match_table(means, used, L0, t, RADIUS, COLOUR_RADIUS)
        pairs = float(P * S)
        if S >= 2:
            assert tie.any(), "the generator promises an exact tie"
            ps, js = np.nonzero(tie)
            a = m[ps[0], js[0]]
            twin = [b for b in range(used[ps[0]]) if b != a and np.array_equal(means[ps[0], L0 + b, 1:], means[ps[0], L0 + a, 1:])
                    and abs(means[ps[0], L0 + b, 0] - means[ps[0], L0 + a, 0]) == 1.0]
            assert twin and a < twin[0], "the tie's winner is the lower of the two slots"
        if P >= 3:
            assert used.min() == 0 and used.max() == S, "u_p must cover 0 and S"
        if P >= 257 and S >= 6:
            assert (m < 0).sum() >= 0.10 * pairs, "at least 10 % of the pairs unmatched"
            assert (passing >= 2).sum() >= 0.05 * pairs, "at least 5 % of the pairs decided between two passing candidates"
    return st


def upload_state(lib, st, weights=None):
    """DeviceFilter(P, L0 + S) holding the planted state: upload_map, grow_enable, upload_landmarks, grow_upload."""
    P, L0, S = st["P"], st["L0"], st["S"]
    L = L0 + S
    f = lib.DeviceFilter(P, L)
    f.upload_map(st["base"], np.tile(np.identity(5).reshape(25), (L, 1)))
    f.grow_enable(L0, 4, 30.0)
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0 if weights is None else weights
    f.upload_poses(poses)
    f.upload_landmarks(0, P, st["means"], st["covs"].reshape(P, L, 25), st["counts"])
    counters = np.zeros((P, 4), dtype=np.int32)
    counters[:, 1] = st["used"]
    counters[:, 2] = L0 + 1 + st["used"]
    f.grow_upload(0, P, counters=counters, slot_ids=st["slot_ids"])
    return f


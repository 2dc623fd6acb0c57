"""The reference of the map-estimate tests: a direct two-pass computation over ALL particles in NumPy float64, and the
comparison with its tolerances.  Shared by test_mapsum_host.py, test_mapsum_gloo.py and test_gpu_mapsum.py.

Tolerances (the issue's): a mean entry to 1e-12 relative -- of the entry, or of its standard deviation in the mixture where the
entry itself is nearer zero than that (a mean of values that cancel has no digits relative to itself); a covariance entry
[i][j] -- total, within or between -- to 1e-10 of sqrt(c_ii c_jj), c the reference's TOTAL covariance; counts and n_eff to 1e-12
relative."""
import numpy as np

POT = 0x40000000  # PK_LANDMARK_POTENTIAL
TRI = np.triu_indices(5)
WITHIN_IJ = ((0, 0), (0, 1), (1, 1), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4))


class Ref(object):
    pass


def two_pass(means, covs, counts, w=None):
    """means (P, L, 5), covs (P, L, 5, 5), counts (P, L) int (the potential bit is masked here), w (P,) or None for ones."""
    means = np.asarray(means, dtype=np.float64)
    P, L = means.shape[:2]
    covs = np.asarray(covs, dtype=np.float64).reshape(P, L, 5, 5)
    w = np.ones(P) if w is None else np.asarray(w, dtype=np.float64).reshape(P)
    r = Ref()
    r.W, r.W2 = w.sum(), (w * w).sum()
    r.mean = np.einsum("p,pli->li", w, means) / r.W
    d = means - r.mean
    r.m2 = np.einsum("p,pli,plj->lij", w, d, d)
    r.between = r.m2 / r.W
    r.wsigma = np.einsum("p,plij->lij", w, covs)
    r.within = r.wsigma / r.W
    r.cov = r.within + r.between
    r.wcount = np.einsum("p,pl->l", w, (np.asarray(counts).astype(np.int64) & ~POT).astype(np.float64))
    r.count = r.wcount / r.W
    r.n_eff = r.W * r.W / r.W2
    return r


def moments_of(means, covs, counts, w=None):
    """One shard's moments (parakeet_slam_amd.mapsum.Moments) from the two-pass computation over ITS particles."""
    from parakeet_slam_amd import mapsum

    r = two_pass(means, covs, counts, w)
    within = np.stack([r.wsigma[:, i, j] for i, j in WITHIN_IJ], axis=1)
    return mapsum.Moments([r.W, r.W2], r.mean, r.m2[:, TRI[0], TRI[1]], within, r.wcount)


def worst(got, ref, rows=None):
    """The largest error of each kind over its tolerance (<= 1 passes), as a dict."""
    sel = slice(None) if rows is None else rows
    sd = np.sqrt(np.einsum("lii->li", ref.cov[sel]))
    out = {}
    out["mean"] = float(np.max(np.abs(got.mean[sel] - ref.mean[sel]) / (1e-12 * np.maximum(np.abs(ref.mean[sel]), sd)), initial=0.0))
    scale = 1e-10 * sd[:, :, None] * sd[:, None, :]
    for name in ("cov", "within", "between"):
        g = getattr(got, "cov" if name == "cov" else "cov_" + name)[sel]
        assert np.array_equal(g, np.swapaxes(g, 1, 2)), name + " is not symmetric"
        out[name] = float(np.max(np.abs(g - getattr(ref, name)[sel]) / scale, initial=0.0))
    out["count"] = float(np.max(np.abs(got.update_count[sel] - ref.count[sel]) / (1e-12 * np.maximum(ref.count[sel], 1.0)), initial=0.0))
    out["n_eff"] = abs(got.n_eff - ref.n_eff) / (1e-12 * ref.n_eff)
    return out


def check(got, ref, rows=None, what=""):
    w = worst(got, ref, rows)
    print("map estimate %s: error / tolerance %s" % (what, {k: "%.3g" % v for k, v in w.items()}))
    assert all(v <= 1.0 for v in w.values()), (what, w)
    return w


def block_diagonal_covs(rs, P, L, scale=0.2):
    """(P, L, 5, 5) symmetric positive definite xy 2x2 (+) rgb 3x3, different in every particle and landmark."""
    c = np.zeros((P, L, 5, 5))
    a = rs.uniform(-0.4, 0.4, size=(P, L, 2, 2))
    c[:, :, :2, :2] = scale * np.identity(2) + a @ np.swapaxes(a, 2, 3)
    b = rs.uniform(-0.4, 0.4, size=(P, L, 3, 3))
    c[:, :, 2:, 2:] = scale * np.identity(3) + b @ np.swapaxes(b, 2, 3)
    return c

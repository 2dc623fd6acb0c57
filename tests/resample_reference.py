"""References for the device resampler (pk_resample), shared by the GPU tests.

``ancestors_match_oracle``: the oracle's float64 resampler on given weights, a few ulp of window.

``ancestors_match_exact``: a stricter one, from the DOWNLOADED log-weights in ``numpy.longdouble``: what systematic
resampling (prkt_core_v2.py:216-250) selects when the weights are summed (nearly) exactly, and a window for the slots where
the device's float64 sums may put a comb point on the other side of a cumulative sum that is derived from the device's
summation order, not measured."""
import math

import numpy as np
import pytest

from oracle.fastslam_oracle import low_variance_ancestors

SCAN_BLOCK = 1024  # kScanBlock: particles per block of the device's scan


def ancestors_match_oracle(anc, w, u):
    """Device ancestors == the oracle's on the same weights.  Ancestors are discrete: the device sums
    the weights in 1024-blocks (Kogge-Stone inside a wave), the reference sequentially, so a comb point
    u r + k r that lies within a few ulp of a cumulative sum may legitimately fall on either side of it
    (expected rate ~ P^2 eps per resample: 1e-6 at P = 1e5).  Anything else is an error."""
    ref = low_variance_ancestors(w, u)
    bad = np.flatnonzero(anc != ref)
    if bad.size == 0:
        return True
    c = np.cumsum(w)
    r = c[-1] / float(len(w))
    for k in bad:
        t = u * r + k * r
        j = min(anc[k], ref[k])
        assert abs(anc[k] - ref[k]) == 1 and abs(t - c[j]) <= 8 * np.finfo(float).eps * c[j], \
            "slot %d: device ancestor %d, oracle %d, comb point %.17g vs cumulative sum %.17g" % (k, anc[k], ref[k], t, c[j])
    assert bad.size <= 2
    return True


def true_weights(logw, domain_is_log):
    """The weights the device means, in longdouble: exp(logw - max) in the log domain (exp(-inf) = 0 when every weight is
    zero: no shift then, as on the device), exp(logw) in the linear one."""
    lw = np.asarray(logw, dtype=np.float64).astype(np.longdouble)
    if domain_is_log:
        m = lw.max()
        if m > -np.inf:
            lw = lw - m
    return np.exp(lw)


def exact_ancestors(logw, u, domain_is_log):
    """(ancestors int64[P], cumulative sums longdouble[P]): first j with C_j >= u r + k r, everything in longdouble, the tail
    clamped to P - 1."""
    w = true_weights(logw, domain_is_log)
    n = w.shape[0]
    c = np.cumsum(w)
    r = c[-1] / np.longdouble(n)
    t = np.longdouble(u) * r + np.arange(n).astype(np.longdouble) * r
    anc = np.minimum(np.searchsorted(c, t, side="left"), n - 1).astype(np.int64)
    return anc, c


def ancestors_match_exact(anc, logw, u, domain_is_log):
    """The device's ancestors against ``exact_ancestors``.  They may differ by +-1, in at most 2 slots, and only where the float64
    comb point lies within (nb + 20) eps C_j of the cumulative sum it straddles, nb = ceil(P / 1024): the device's C_j carries
    4 + 6 + 3 additions inside its block (four particles of a lane, six Kogge-Stone steps, three wave totals), nb sequential
    additions of block totals, one rounding in off + clocal and one ulp of the device's exp per term; its comb point three
    roundings -- nb + 18 roundings of at most eps C_j / 2 each, so the window has a factor two to spare.  Returns the number of
    differing slots."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy.longdouble is no wider than float64 here: no exact resampler to compare with")
    anc = np.asarray(anc, dtype=np.int64)
    ref, c = exact_ancestors(logw, u, domain_is_log)
    n = anc.shape[0]
    assert anc.min() >= 0 and anc.max() <= n - 1
    bad = np.flatnonzero(anc != ref)
    if bad.size == 0:
        return 0
    nb = int(math.ceil(n / float(SCAN_BLOCK)))
    eps = np.finfo(np.float64).eps
    r = float(c[-1]) / float(n)
    for k in bad:
        t = u * r + float(k) * r  # the float64 comb point
        j = min(anc[k], ref[k])   # the cumulative sum the two verdicts straddle
        cj = float(c[j])
        assert abs(anc[k] - ref[k]) == 1, "slot %d: device ancestor %d, exact %d" % (k, anc[k], ref[k])
        assert abs(t - cj) <= (nb + 20) * eps * cj, \
            "slot %d: device ancestor %d, exact %d, comb point %.17g vs cumulative sum %.17g (window %d eps)" % (
                k, anc[k], ref[k], t, cj, nb + 20)
    assert bad.size <= 2, "%d slots differ from the exact resampler" % bad.size
    return int(bad.size)

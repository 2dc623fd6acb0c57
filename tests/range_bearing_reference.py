"""Range-bearing blobs under the bearing model (pk_scan_ranges; DESIGN.md section 4, "Range-bearing scans") in NumPy, float64 -- the
yardstick of tests/test_range_bearing_host.py and tests/test_gpu_range_bearing.py.  TEST INFRASTRUCTURE ONLY.

Built on bearing_model_reference by import: a blob whose range is NaN goes through that module's functions, call for call, so an
oracle given no finite range IS BearingOracle.  A blob with a range is handled here, in dense algebra with np.linalg -- 2x2 matrices
built from outer products for the association, one 5x5 measurement (bearing, range, r, g, b) for the update -- so that the device's
factored form (a closed-form 2x2 inverse beside the colour block's 3x3) is held to something that does not share it.

    u = R(h) unit(cos beta, sin beta), n = (-uy, ux), m = s + rho u
    position    N(m; mu_xy, Sigma_xy + q_rho u u' + rho^2 q00 n n')
    update      z = (beta, rho, r, g, b); H rows (-dy / q, dx / q, 0, 0, 0), (dx / r, dy / r, 0, 0, 0), identity on the colours (the
                first two rows zero at q = 0); R = diag(q00, q_rho) (+) Qt[1:, 1:]; innovation (wrap(beta - zhat0), rho - r, colours)
    weight      log w = -5/2 log 2 pi - 1/2 log det S - 1/2 d' S^-1 d
"""
import math

import numpy as np

from oracle.fastslam_oracle import BEARING_GATE, COLOR_GATE, NO_MATCH_WEIGHT, TWO_PI, prob_color_match

import bearing_model_reference as bearing
from bearing_model_reference import BearingOracle, world_ray, wrap


def measured_point_covariance(cov_xy, ux, uy, rho, q_rho, q00):
    """Sigma_xy + q_rho u u' + rho^2 q00 n n', batched over the leading dims of cov_xy (..., 2, 2) and of the ray."""
    u = np.stack([ux, uy], axis=-1)
    n = np.stack([-uy, ux], axis=-1)
    return cov_xy + q_rho * u[..., :, None] * u[..., None, :] + (rho * rho * q00) * n[..., :, None] * n[..., None, :]


def prob_position_match(fx, fy, cov_xy, sx, sy, sh, bearing_, rho, q_rho, q00):
    """The 2x2 density at the measured point; cov_xy (..., 2, 2)."""
    ux, uy = world_ray(bearing_, sh)
    ux, uy = np.broadcast_to(ux, np.shape(fx)), np.broadcast_to(uy, np.shape(fx))
    S = measured_point_covariance(cov_xy, ux, uy, rho, q_rho, q00)
    e = np.stack([sx + rho * ux - fx, sy + rho * uy - fy], axis=-1)
    with np.errstate(all="ignore"):
        sign, logdet = np.linalg.slogdet(S)
        maha = np.einsum("...i,...ij,...j->...", e, np.linalg.inv(S), e)
        return np.where(sign > 0, np.exp(-0.5 * (2.0 * math.log(TWO_PI) + logdet + maha)), np.nan)


def probability_of_match(sx, sy, sh, blob, rho, q_rho, q00, mean, cov):
    """bearing_model_reference.probability_of_match for a blob with a range: the same gates, the position factor above."""
    fx, fy = mean[..., 0], mean[..., 1]
    expected = np.arctan2(fy - sy, fx - sx) - sh
    delb = wrap(blob[0] - expected)
    cd = np.power(blob[1] - mean[..., 2], 2) + np.power(blob[2] - mean[..., 3], 2) + np.power(blob[3] - mean[..., 4], 2)
    bp = 500.0 * prob_position_match(fx, fy, cov[..., :2, :2], sx, sy, sh, blob[0], rho, q_rho, q00)
    cp = 500.0 * prob_color_match((mean[..., 2], mean[..., 3], mean[..., 4]),
                                  (cov[..., 2, 2], cov[..., 2, 3], cov[..., 2, 4], cov[..., 3, 3], cov[..., 3, 4], cov[..., 4, 4]),
                                  (blob[1], blob[2], blob[3]))
    p = bp * cp / 250000.0
    p = np.where(np.abs(cd) > COLOR_GATE, 0.0, p)
    p = np.where(np.abs(delb) > BEARING_GATE, 0.0, p)
    return p


def predicted_measurement(sx, sy, sh, mean):
    """(bearing, range, r, g, b) a landmark at `mean` is expected to show from the pose: what H is the Jacobian of."""
    dx, dy = mean[..., 0] - sx, mean[..., 1] - sy
    return np.stack([np.arctan2(dy, dx) - sh, np.sqrt(dx * dx + dy * dy), mean[..., 2], mean[..., 3], mean[..., 4]], axis=-1)


def measurement_noise(Qt, q_rho):
    R = np.zeros((5, 5))
    R[0, 0] = Qt[0, 0]
    R[1, 1] = q_rho
    R[2:, 2:] = Qt[1:, 1:]
    return R


def ekf_update_dense(sx, sy, sh, mean, cov, blob, rho, q_rho, Qt):
    """One ranged observation of one landmark, batched over leading dims: (new_mean, new_cov, logweight, aux)."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    lead = mean.shape[:-1]
    dx, dy = mean[..., 0] - sx, mean[..., 1] - sy
    q = np.power(dx, 2) + np.power(dy, 2)
    r = np.sqrt(q)
    zhat = predicted_measurement(sx, sy, sh, mean)
    H = np.zeros(lead + (5, 5))
    with np.errstate(all="ignore"):
        H[..., 0, 0] = np.where(q == 0, 0.0, -dy / q)
        H[..., 0, 1] = np.where(q == 0, 0.0, dx / q)
        H[..., 1, 0] = np.where(q == 0, 0.0, dx / r)
        H[..., 1, 1] = np.where(q == 0, 0.0, dy / r)
    H[..., 2, 2] = H[..., 3, 3] = H[..., 4, 4] = 1.0
    Ht = np.swapaxes(H, -1, -2)
    S = H @ cov @ Ht + measurement_noise(np.asarray(Qt, dtype=np.float64), q_rho)
    Sinv = np.linalg.inv(S)
    K = cov @ Ht @ Sinv
    z = np.array([blob[0], rho, blob[1], blob[2], blob[3]], dtype=np.float64)
    delz = np.broadcast_to(z, zhat.shape) - zhat
    delz = np.concatenate([wrap(delz[..., :1]), delz[..., 1:]], axis=-1)
    new_mean = mean + np.einsum("...ij,...j->...i", K, delz)
    new_cov = (np.identity(5) - K @ H) @ cov
    _, logdet = np.linalg.slogdet(S)
    logweight = -2.5 * math.log(TWO_PI) - 0.5 * logdet - 0.5 * np.einsum("...i,...ij,...j->...", delz, Sinv, delz)
    return new_mean, new_cov, logweight, dict(zhat=zhat, H=H, S=S, K=K, delz=delz)


def _rows(B, ranges, variances):
    r = np.full(B, np.nan) if ranges is None else np.asarray(ranges, dtype=np.float64).reshape(B)
    v = np.full(B, np.nan) if variances is None else np.asarray(variances, dtype=np.float64).reshape(B)
    return r, v


class RangeBearingOracle(BearingOracle):
    """BearingOracle whose associate / observe take a range and a variance per blob (NaN range: none -- the parent's own code).

    It keeps, over every association it has made, what the GPU tests need to know about how close its verdicts were:
    min_rel_gap       the smallest (best - second best) / best over the (particle, blob) pairs that were matched while a second
                      landmark had a probability > 0 (inf: never);
    min_gate_margins  the smallest | |wrapped bearing difference| - 0.5 | and | squared colour distance - 300 | met."""

    def __init__(self, *a, **k):
        super(RangeBearingOracle, self).__init__(*a, **k)
        self.min_rel_gap = np.inf
        self.min_gate_margins = [np.inf, np.inf]

    def gate_margins(self, blobs):
        """bearing_model_reference.gate_margins of every blob against the current state: (bearing, colour) minima."""
        sx, sy, sh = self.x[:, None], self.y[:, None], self.h[:, None]
        mb = mc = np.inf
        for b in range(len(blobs)):
            g = bearing.gate_margins(sx, sy, sh, blobs[b], self.mean)
            mb, mc = min(mb, float(g[0].min())), min(mc, float(g[1].min()))
        return mb, mc

    def associate(self, blobs, ranges=None, variances=None, chunk=256):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = blobs.shape[0]
        rng, var = _rows(B, ranges, variances)
        ids = np.zeros((self.P, B), dtype=np.int32)
        if self.L == 0:
            return ids
        if B:
            mb, mc = self.gate_margins(blobs)
            self.min_gate_margins = [min(self.min_gate_margins[0], mb), min(self.min_gate_margins[1], mc)]
        for p0 in range(0, self.P, chunk):
            p1 = min(self.P, p0 + chunk)
            sx, sy, sh = self.x[p0:p1, None], self.y[p0:p1, None], self.h[p0:p1, None]
            for b in range(B):
                if np.isnan(rng[b]):
                    pr = bearing.probability_of_match(sx, sy, sh, blobs[b], self.mean[p0:p1], self.cov[p0:p1])
                else:
                    pr = probability_of_match(sx, sy, sh, blobs[b], rng[b], var[b], self.Qt[0, 0], self.mean[p0:p1], self.cov[p0:p1])
                pr = np.where(np.isnan(pr), 0.0, pr)
                best = np.argmax(pr, axis=1)
                pmax = pr[np.arange(p1 - p0), best]
                ids[p0:p1, b] = np.where(pmax > 0.0, best + 1, 0)
                if self.L > 1:
                    second = np.partition(pr, -2, axis=1)[:, -2]
                    m = (pmax > 0.0) & (second > 0.0)
                    if m.any():
                        self.min_rel_gap = min(self.min_rel_gap, float(((pmax[m] - second[m]) / pmax[m]).min()))
        return ids

    def observe(self, blobs, ids=None, ranges=None, variances=None):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = blobs.shape[0]
        rng, var = _rows(B, ranges, variances)
        if ids is None:
            ids = self.associate(blobs, rng, var)
        ids = np.asarray(ids, dtype=np.int64)
        if ids.ndim == 1:
            ids = np.broadcast_to(ids, (self.P, B))
        ar = np.arange(self.P)
        for b in range(B):
            idb = ids[:, b]
            m = idb > 0
            self.logw[~m] += math.log(NO_MATCH_WEIGHT)
            self.n_unmatched[~m] += 1
            if not m.any():
                continue
            pi, li = ar[m], idb[m] - 1
            if np.isnan(rng[b]):
                nm, nc, lw, _ = bearing.ekf_update_dense(self.x[pi], self.y[pi], self.h[pi], self.mean[pi, li], self.cov[pi, li], blobs[b], self.Qt)
            else:
                nm, nc, lw, _ = ekf_update_dense(self.x[pi], self.y[pi], self.h[pi], self.mean[pi, li], self.cov[pi, li], blobs[b],
                                                 rng[b], var[b], self.Qt)
            mut = ~self.immutable[li]
            self.mean[pi[mut], li[mut]] = nm[mut]
            self.cov[pi[mut], li[mut]] = nc[mut]
            self.count[pi[mut], li[mut]] += 2
            pot = self.potential[pi, li]
            self.logw[pi] += np.where(pot, math.log(NO_MATCH_WEIGHT), lw)
            promote = pot & (self.count[pi, li] > 5)
            self.potential[pi[promote], li[promote]] = False
        return ids


def range_scan(world_means, pose, rs=None, sigma0=0.0, sigma1=0.0, every=None):
    """The ranges that go with wrapped_scan(world_means, pose, ...): the true distances, with noise of sigma0 + sigma1 rho drawn from
    `rs` (a stream of its own, so that the bearings of a run with ranges are those of the run without), and the variances
    (sigma0 + sigma1 rho)^2 of the REPORTED range, as the facade forms them.  every = k: blobs k - 1, 2k - 1, ... have no range."""
    x, y, _ = pose
    rho = np.hypot(world_means[:, 0] - x, world_means[:, 1] - y)
    if rs is not None:
        rho = rho + (sigma0 + sigma1 * rho) * rs.standard_normal(len(rho))
    if every:
        rho[every - 1::every] = np.nan
    sig = sigma0 + sigma1 * rho
    return rho, sig * sig

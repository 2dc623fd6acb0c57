"""The bearing measurement model (pk_set_measurement_model(f, PK_MODEL_BEARING); DESIGN.md section 4, "The bearing model") in NumPy,
float64 -- the yardstick of tests/test_bearing_model_host.py and tests/test_gpu_bearing_model.py.  TEST INFRASTRUCTURE ONLY.

Dense 4x4 / 5x5 algebra with np.linalg, written the way oracle.fastslam_oracle.ekf_update_dense writes the reference's, so that
the device's factored form (a scalar and a 3x3 problem, det Q = Q00 det(C + Qc)) is held to something that does not share it.

    wrap(a) = a - 2 pi rint(a / 2 pi)                      the identity, exactly, inside (-pi, pi)
    gate        |wrap(beta - (atan2(dy, dx) - h))| > 0.5 -> 0;  squared colour distance > 300 -> 0
    position    ray = R(h) unit(cos beta, sin beta); closest point on the LINE through the robot; 2x2 density there
    update      zhat0 = atan2(dy, dx) - h; delta0 = wrap(beta - zhat0); H row 0 = (-dy / q, dx / q), (0, 0) at q = 0
    weight      log w = -2 log 2 pi - 1/2 log det Q - 1/2 delta' Q^-1 delta
"""
import math

import numpy as np

from oracle.fastslam_oracle import (BEARING_GATE, COLOR_GATE, NO_MATCH_WEIGHT, TWO_PI, GrowingOracle, OracleFilter, mvn_pdf_2,
                                    prob_color_match)


def wrap(a):
    a = np.asarray(a, dtype=np.float64)
    return a - TWO_PI * np.rint(a / TWO_PI)


def world_ray(bearing, sh):
    """The blob's unit ray (utils.unit of (cos b, sin b, 0), as closest_point forms it) turned by the heading."""
    cb, sb = np.cos(bearing), np.sin(bearing)
    length = np.sqrt(cb * cb + sb * sb + 0.0)
    ux, uy = cb * (1.0 / length), sb * (1.0 / length)
    ch, sn = np.cos(sh), np.sin(sh)
    return ux * ch - uy * sn, ux * sn + uy * ch


def prob_position_match(fx, fy, cov_xy, sx, sy, sh, bearing):
    wx, wy = world_ray(bearing, sh)
    ox, oy = fx - sx, fy - sy
    mag = ox * wx + oy * wy + 0.0 * 0.0
    nx, ny = sx + wx * mag, sy + wy * mag
    with np.errstate(all="ignore"):
        return mvn_pdf_2(nx - fx, ny - fy, *cov_xy)


def probability_of_match(sx, sy, sh, blob, mean, cov):
    """oracle.probability_of_match under the bearing model, broadcast the same way."""
    fx, fy = mean[..., 0], mean[..., 1]
    expected = np.arctan2(fy - sy, fx - sx) - sh
    delb = wrap(blob[0] - expected)
    cd = np.power(blob[1] - mean[..., 2], 2) + np.power(blob[2] - mean[..., 3], 2) + np.power(blob[3] - mean[..., 4], 2)
    bp = 500.0 * prob_position_match(fx, fy, (cov[..., 0, 0], cov[..., 0, 1], cov[..., 1, 1]), sx, sy, sh, blob[0])
    cp = 500.0 * prob_color_match((mean[..., 2], mean[..., 3], mean[..., 4]),
                                  (cov[..., 2, 2], cov[..., 2, 3], cov[..., 2, 4], cov[..., 3, 3], cov[..., 3, 4], cov[..., 4, 4]),
                                  (blob[1], blob[2], blob[3]))
    p = bp * cp / 250000.0
    p = np.where(np.abs(cd) > COLOR_GATE, 0.0, p)
    p = np.where(np.abs(delb) > BEARING_GATE, 0.0, p)
    return p


def gate_margins(sx, sy, sh, blob, mean):
    """(| |wrapped bearing difference| - 0.5 |, | squared colour distance - 300 |) of every pair: how far each gate's verdict is from
    turning over (the GPU tests draw their scenes so that rounding cannot turn one)."""
    delb = wrap(blob[0] - (np.arctan2(mean[..., 1] - sy, mean[..., 0] - sx) - sh))
    cd = np.power(blob[1] - mean[..., 2], 2) + np.power(blob[2] - mean[..., 3], 2) + np.power(blob[3] - mean[..., 4], 2)
    return np.abs(np.abs(delb) - BEARING_GATE), np.abs(cd - COLOR_GATE)


def ekf_update_dense(sx, sy, sh, mean, cov, blob, Qt):
    """One observation of one landmark under the bearing model, batched over leading dims: (new_mean, new_cov, logweight, aux)."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    lead = mean.shape[:-1]
    fx, fy = mean[..., 0], mean[..., 1]
    dx, dy = fx - sx, fy - sy
    q = np.power(dx, 2) + np.power(dy, 2)
    zhat = np.stack([np.arctan2(dy, dx) - sh, mean[..., 2], mean[..., 3], mean[..., 4]], axis=-1)
    with np.errstate(all="ignore"):
        h0 = np.where(q == 0, 0.0, -dy / q)
        h1 = np.where(q == 0, 0.0, dx / q)
    H = np.zeros(lead + (4, 5))
    H[..., 0, 0] = h0
    H[..., 0, 1] = h1
    H[..., 1, 2] = H[..., 2, 3] = H[..., 3, 4] = 1.0
    Ht = np.swapaxes(H, -1, -2)
    Q = H @ cov @ Ht + Qt
    Qinv = np.linalg.inv(Q)
    K = cov @ Ht @ Qinv
    delz = np.broadcast_to(np.asarray(blob, dtype=np.float64), zhat.shape) - zhat
    delz = np.concatenate([wrap(delz[..., :1]), delz[..., 1:]], axis=-1)
    new_mean = mean + np.einsum("...ij,...j->...i", K, delz)
    new_cov = (np.identity(5) - K @ H) @ cov
    _, logdet = np.linalg.slogdet(Q)
    logweight = -2.0 * math.log(TWO_PI) - 0.5 * logdet - 0.5 * np.einsum("...i,...ij,...j->...", delz, Qinv, delz)
    return new_mean, new_cov, logweight, dict(zhat=zhat, H=H, Q=Q, K=K, delz=delz)


class BearingOracle(OracleFilter):
    """OracleFilter whose association and update are the bearing model's; everything else -- motion, resampling, summary, the
    potential-feature rule -- is the parent's."""

    def associate(self, blobs, chunk=256):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = blobs.shape[0]
        ids = np.zeros((self.P, B), dtype=np.int32)
        if self.L == 0:
            return ids
        for p0 in range(0, self.P, chunk):
            p1 = min(self.P, p0 + chunk)
            sx, sy, sh = self.x[p0:p1, None], self.y[p0:p1, None], self.h[p0:p1, None]
            for b in range(B):
                pr = probability_of_match(sx, sy, sh, blobs[b], self.mean[p0:p1], self.cov[p0:p1])
                pr = np.where(np.isnan(pr), 0.0, pr)
                best = np.argmax(pr, axis=1)
                pmax = pr[np.arange(p1 - p0), best]
                ids[p0:p1, b] = np.where(pmax > 0.0, best + 1, 0)
        return ids

    def observe(self, blobs, ids=None):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = blobs.shape[0]
        if ids is None:
            ids = self.associate(blobs)
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
            nm, nc, lw, _ = ekf_update_dense(self.x[pi], self.y[pi], self.h[pi], self.mean[pi, li], self.cov[pi, li], blobs[b], self.Qt)
            mut = ~self.immutable[li]
            self.mean[pi[mut], li[mut]] = nm[mut]
            self.cov[pi[mut], li[mut]] = nc[mut]
            self.count[pi[mut], li[mut]] += 2
            pot = self.potential[pi, li]
            self.logw[pi] += np.where(pot, math.log(NO_MATCH_WEIGHT), lw)
            promote = pot & (self.count[pi, li] > 5)
            self.potential[pi[promote], li[promote]] = False
        return ids


def under_bearing_model(growing):
    """A GrowingOracle (or a subclass of it: RetiringOracle) whose filter runs the bearing model: the bookkeeping is untouched --
    it already triangulates with heading + bearing."""
    assert isinstance(growing, GrowingOracle) and type(growing.f) is OracleFilter
    growing.f.__class__ = BearingOracle  # (BearingOracle adds no state)
    return growing


def wrapped_scan(world_means, pose, rs=None, sigma_bearing=0.0, sigma_colour=0.0):
    """synthetic_scan with the bearings wrapped into [-pi, pi], as a sensor reports them, and optional noise."""
    x, y, h = pose
    B = world_means.shape[0]
    blobs = np.empty((B, 4))
    blobs[:, 0] = np.arctan2(world_means[:, 1] - y, world_means[:, 0] - x) - h
    blobs[:, 1:] = world_means[:, 2:]
    if rs is not None:
        blobs[:, 0] += sigma_bearing * rs.standard_normal(B)
        blobs[:, 1:] += sigma_colour * rs.standard_normal((B, 3))
    blobs[:, 0] = wrap(blobs[:, 0])
    return blobs

"""The measurement-informed proposal (pk_propose / pk_propose_odom; DESIGN.md section 4, "The measurement-informed proposal") in
NumPy, float64 -- the yardstick of tests/test_proposal_reference_host.py and tests/test_gpu_proposal.py.  TEST INFRASTRUCTURE ONLY.

Dense algebra with np.linalg: Lambda, m and R come from np.linalg.solve / cholesky, and the weight increment is computed
INDEPENDENTLY of the device's formula -- as the log-density of the stacked n-vector nu under N(0, D + A A') with slogdet and solve
on the n x n matrix, plus the colour densities -- so that the device's 3 x 3 form (Woodbury, the determinant lemma) is held to
something that does not share it.  `delta_formula` restates the 3 x 3 form for the host test that compares the two.
"""
import math

import numpy as np

import odom_reference as odo
from bearing_model_reference import BearingOracle, gate_margins, wrap
from oracle.fastslam_oracle import NO_MATCH_WEIGHT, OracleFilter, wrap_heading

LOG_2PI = math.log(2.0 * math.pi)
LOG_LOW = math.log(NO_MATCH_WEIGHT)


# ------------------------------------------------------------------------------------------------------------ the motion models
def twist(v, w, dt):
    return ("twist", float(v), float(w), float(dt))


def odom(delta, alphas):
    return ("odom", np.asarray(delta, dtype=np.float64), np.asarray(alphas, dtype=np.float64))


def control_sigmas(control):
    if control[0] == "twist":
        sd, sh = OracleFilter.motion_sigmas(control[1], control[2])
        return np.array([sd, sh, sh])
    return odo.sigmas(control[1], control[2])


def move(x, y, h, control, n):
    """g(x-, u, n): the oracle's own motion functions with the SCALED noises n (P, 3)."""
    n = np.asarray(n, dtype=np.float64).reshape(-1, 3)
    if control[0] == "twist":
        _, v, w, dt = control
        dh = w * dt
        ds = v * dt + (0.0 + n[:, 0])
        h1 = h + dh / 2 + (0.0 + n[:, 1])
        h2 = h1 + dh / 2 + (0.0 + n[:, 2])
        return x + ds * np.cos(h1), y + ds * np.sin(h1), wrap_heading(h2)
    return odo._sample(x, y, h, control[1], np.ones(3), n, np.float64)


def noise_jacobian(control, hhat):
    """G = d pose / d n at n = 0 from the predicted heading and the control alone: (P, 3, 3), G[:, :, k] = column k."""
    hhat = np.asarray(hhat, dtype=np.float64)
    G = np.zeros(hhat.shape + (3, 3))
    if control[0] == "twist":
        _, v, w, dt = control
        h1, ds = hhat - w * dt / 2, v * dt
        G[..., 0, 0], G[..., 1, 0] = np.cos(h1), np.sin(h1)
        G[..., 0, 1], G[..., 1, 1], G[..., 2, 1] = -ds * np.sin(h1), ds * np.cos(h1), 1.0
        G[..., 2, 2] = 1.0
    else:
        d = control[1]
        h1, t = hhat - d[2], d[1]
        G[..., 0, 0], G[..., 1, 0], G[..., 2, 0] = t * np.sin(h1), -t * np.cos(h1), -1.0
        G[..., 0, 1], G[..., 1, 1] = -np.cos(h1), -np.sin(h1)
        G[..., 2, 2] = -1.0
    return G


# ------------------------------------------------------------------------------------------------------------ the two weights
def delta_dense(A, D, nu, kappa_terms, low):
    """The weight increment as a density: nu (n,) under N(0, diag(D) + A A'), the n colour densities (each
    log det(C + Qc) + d' (C + Qc)^-1 d, in kappa_terms), `low` blobs that weigh log 0.1."""
    n = len(nu)
    out = low * LOG_LOW
    if n:
        S = np.diag(D) + A @ A.T
        _, logdet = np.linalg.slogdet(S)
        out += -0.5 * n * LOG_2PI - 0.5 * logdet - 0.5 * float(nu @ np.linalg.solve(S, nu))
        out += float(np.sum(-1.5 * LOG_2PI - 0.5 * np.asarray(kappa_terms)))
    return out


def delta_formula(A, D, nu, kappa_terms, low):
    """The same by the 3 x 3 form the device uses: (delta, Lambda, eta)."""
    n = len(nu)
    Lam, eta = np.identity(3), np.zeros(3)
    c = ell = 0.0
    for i in range(n):
        Lam += np.outer(A[i], A[i]) / D[i]
        eta += A[i] * nu[i] / D[i]
        c += nu[i] * nu[i] / D[i]
        ell += math.log(D[i])
    m = np.linalg.solve(Lam, eta)
    _, logdet = np.linalg.slogdet(Lam)
    kappa = float(np.sum(kappa_terms)) if n else 0.0
    return -2.0 * n * LOG_2PI - 0.5 * (ell + logdet) - 0.5 * (c - float(eta @ m)) - 0.5 * kappa + low * LOG_LOW, Lam, eta


def n_eff(logw):
    w = np.exp(logw - np.max(logw))
    return float(np.sum(w) ** 2 / np.sum(w * w))


# ------------------------------------------------------------------------------------------------------------ the filter
class ProposalOracle(BearingOracle):
    """BearingOracle whose step draws the pose from the motion model conditioned on the scan.  propose() leaves, for the tests:
    xi (P, 3), dlogw (P,), used (P,), Lambda (P, 3, 3), xhat (the predicted poses, (P, 3)) and ids (the settled ids, (P, B))."""

    def matches(self, xhat, control, s, blobs, ids):
        """Per particle the rows of its settled matches: lists of (A (n, 3), D (n,), nu (n,), kappa terms (n,), low)."""
        P, B = self.P, len(blobs)
        sx, sy, sh = xhat
        G = noise_jacobian(control, sh)
        Qc = self.Qt[1:, 1:]
        A = np.zeros((P, B, 3))
        D, NU, KAP = np.zeros((P, B)), np.zeros((P, B)), np.zeros((P, B))
        settled = np.zeros((P, B), dtype=bool)
        for b in range(B):
            idb = ids[:, b]
            li = np.maximum(idb - 1, 0)
            ar = np.arange(P)
            mean, cov = self.mean[ar, li], self.cov[ar, li]
            settled[:, b] = (idb > 0) & ~self.potential[ar, li]
            dx, dy = mean[:, 0] - sx, mean[:, 1] - sy
            q = dx * dx + dy * dy
            with np.errstate(all="ignore"):
                hx = np.stack([np.where(q == 0, 0.0, dy / q), np.where(q == 0, 0.0, -dx / q), np.where(q == 0, 0.0, -1.0)], axis=-1)
            hm = -hx[:, :2]
            NU[:, b] = wrap(blobs[b, 0] - (np.arctan2(dy, dx) - sh))
            D[:, b] = np.einsum("pi,pij,pj->p", hm, cov[:, :2, :2], hm) + self.Qt[0, 0]
            A[:, b] = s * np.einsum("pik,pi->pk", G, hx)
            C = cov[:, 2:, 2:] + Qc
            dc = blobs[b, 1:] - mean[:, 2:]
            KAP[:, b] = np.linalg.slogdet(C)[1] + np.einsum("pi,pi->p", dc, np.linalg.solve(C, dc[..., None])[..., 0])
        out = []
        for p in range(P):
            k = settled[p]
            out.append((A[p, k], D[p, k], NU[p, k], KAP[p, k], int(B - k.sum())))
        return out

    def propose(self, control, z, blobs, ids=None, fresh=True):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        z = np.asarray(z, dtype=np.float64).reshape(self.P, 3)
        P, B = self.P, len(blobs)
        s = control_sigmas(control)
        x0, y0, h0 = self.x.copy(), self.y.copy(), self.h.copy()
        xhat = move(x0, y0, h0, control, np.zeros((P, 3)))
        # association at the predicted pose, against the untouched landmarks
        self.x, self.y, self.h = xhat
        if ids is None:
            ids = self.associate(blobs) if B else np.zeros((P, 0), dtype=np.int32)
        else:
            ids = np.asarray(ids, dtype=np.int32)  # one row for every particle, or (P, B)
            ids = (ids if ids.ndim == 2 else np.broadcast_to(ids.reshape(1, B), (P, B))).copy()
        rows = self.matches(xhat, control, s, blobs, ids)
        self.xi, self.dlogw, self.used = np.empty((P, 3)), np.empty(P), np.empty(P, dtype=np.int32)
        self.Lambda = np.empty((P, 3, 3))
        for p, (A, D, nu, kap, low) in enumerate(rows):
            Lam = np.identity(3) + (A.T / D) @ A if len(nu) else np.identity(3)
            eta = (A.T / D) @ nu if len(nu) else np.zeros(3)
            self.Lambda[p] = Lam
            if len(nu):
                R = np.linalg.cholesky(Lam)
                self.xi[p] = np.linalg.solve(Lam, eta) + np.linalg.solve(R.T, z[p])
            else:
                self.xi[p] = z[p]
            self.dlogw[p] = delta_dense(A, D, nu, kap, low)
            self.used[p] = len(nu)
        self.xhat = np.stack(xhat, axis=1)
        self.ids = ids
        # the move, with the normals xi; the update at the sampled pose with the settled ids; the weight from the proposal alone
        self.x, self.y, self.h = move(x0, y0, h0, control, s * self.xi)
        logw0 = np.zeros(P) if fresh else self.logw.copy()
        self.observe(blobs, ids)
        self.logw = logw0 + self.dlogw
        return ids

    def margins_at_prediction(self, control, blobs):
        """The smallest gate margins (bearing, colour) of every (particle, landmark, blob) at the predicted poses of the CURRENT
        state (call before propose)."""
        xh = move(self.x, self.y, self.h, control, np.zeros((self.P, 3)))
        mb = mc = np.inf
        for b in range(len(blobs)):
            a, c = gate_margins(xh[0][:, None], xh[1][:, None], xh[2][:, None], blobs[b], self.mean)
            mb, mc = min(mb, float(a.min())), min(mc, float(c.min()))
        return mb, mc

"""Ranges in the measurement-informed proposal (pk_proposal_ranges; DESIGN.md section 4, "Ranges in the proposal") in NumPy, float64 --
the yardstick of tests/test_range_proposal_host.py and tests/test_gpu_range_proposal.py.  TEST INFRASTRUCTURE ONLY.

Composed of range_bearing_reference and proposal_reference by import: RangedProposalOracle IS both oracles (it inherits the
association, the update and the margins it keeps from RangeBearingOracle, the motion functions, the noise Jacobian and the rows of
an unranged match from ProposalOracle), and a step in which no blob has a finite range is ProposalOracle.propose itself, call for
call.  What is new is written here in dense algebra with np.linalg: a ranged match contributes TWO stacked innovations (bearing,
range) with the 2 x 2 variance S2 = h_m Sigma_xy h_m' + diag(q00, q_rho) and the 2 x 3 block A = (h_x G) s; Lambda, m and R come
from np.linalg.solve / cholesky on the stacked rows, and the weight increment is computed INDEPENDENTLY of the device's formula --
the log-density of the stacked vector under N(0, D + A A'), D block diagonal in 1 x 1 and 2 x 2 blocks, with slogdet and solve on
the full matrix -- so that the device's 3 x 3 form with its closed-form 2 x 2 inverses is held to something that does not share
it.  `delta_formula_blocks` restates that 3 x 3 form for the host test that compares the two.
"""
import math

import numpy as np

import proposal_reference as pr
import range_bearing_reference as rref
from bearing_model_reference import wrap
from proposal_reference import LOG_2PI, LOG_LOW, ProposalOracle
from range_bearing_reference import RangeBearingOracle


# ------------------------------------------------------------------------------------------------------------ the two weights
def block_diagonal(blocks):
    n = sum(len(b) for b in blocks)
    D = np.zeros((n, n))
    i = 0
    for b in blocks:
        m = len(b)
        D[i:i + m, i:i + m] = b
        i += m
    return D


def delta_dense_blocks(A, blocks, nu, kappa_terms, low):
    """The weight increment as a density: the stacked nu (rows,) under N(0, blockdiag(blocks) + A A'), one colour density per MATCH
    (kappa_terms: log det(C + Qc) + d' (C + Qc)^-1 d each), `low` blobs that weigh log 0.1."""
    rows = len(nu)
    out = low * LOG_LOW
    if rows:
        S = block_diagonal(blocks) + A @ A.T
        _, logdet = np.linalg.slogdet(S)
        out += -0.5 * rows * LOG_2PI - 0.5 * logdet - 0.5 * float(nu @ np.linalg.solve(S, nu))
        out += float(np.sum(-1.5 * LOG_2PI - 0.5 * np.asarray(kappa_terms)))
    return out


def delta_formula_blocks(A, blocks, nu, kappa_terms, low):
    """The same by the 3 x 3 form the device uses, match by match, the 2 x 2 blocks inverted in closed form: (delta, Lambda, eta)."""
    Lam, eta = np.identity(3), np.zeros(3)
    c = ell = 0.0
    n = n_rho = 0
    i = 0
    for blk in blocks:
        if len(blk) == 1:
            d = blk[0][0]
            Lam += np.outer(A[i], A[i]) / d
            eta += A[i] * nu[i] / d
            c += nu[i] * nu[i] / d
            ell += math.log(d)
        else:
            s00, s01, s11 = blk[0][0], blk[0][1], blk[1][1]
            det = s00 * s11 - s01 * s01
            inv = np.array([[s11, -s01], [-s01, s00]]) / det
            A2, v = A[i:i + 2], nu[i:i + 2]
            Lam += A2.T @ inv @ A2
            eta += A2.T @ inv @ v
            c += float(v @ inv @ v)
            ell += math.log(det)
            n_rho += 1
        n += 1
        i += len(blk)
    m = np.linalg.solve(Lam, eta)
    _, logdet = np.linalg.slogdet(Lam)
    kappa = float(np.sum(kappa_terms)) if n else 0.0
    delta = -(2.0 * n + 0.5 * n_rho) * LOG_2PI - 0.5 * (ell + logdet) - 0.5 * (c - float(eta @ m)) - 0.5 * kappa + low * LOG_LOW
    return delta, Lam, eta


# ------------------------------------------------------------------------------------------------------------ a ranged match
def pose_jacobian(sx, sy, mean):
    """h_x (..., 2, 3): the derivative of range_bearing_reference.predicted_measurement's (bearing, range) in the POSE (x, y, h):
    [[dy / q, -dx / q, -1], [-dx / r, -dy / r, 0]], all zero at q = 0 (as the update has its own H there)."""
    dx, dy = mean[..., 0] - sx, mean[..., 1] - sy
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    H = np.zeros(np.shape(q) + (2, 3))
    with np.errstate(all="ignore"):
        H[..., 0, 0] = np.where(q == 0, 0.0, dy / q)
        H[..., 0, 1] = np.where(q == 0, 0.0, -dx / q)
        H[..., 0, 2] = np.where(q == 0, 0.0, -1.0)
        H[..., 1, 0] = np.where(q == 0, 0.0, -dx / r)
        H[..., 1, 1] = np.where(q == 0, 0.0, -dy / r)
    return H


class RangedProposalOracle(ProposalOracle, RangeBearingOracle):
    """ProposalOracle whose step takes a range and a variance per blob (NaN range: none).  propose() leaves what ProposalOracle's
    leaves -- xi, dlogw, used (MATCHES, not rows), Lambda, xhat, ids -- and n_rho (P,), the matches that carried a range."""

    def ranged_rows(self, xhat, control, s, blobs, rng, var, ids):
        """Per particle the stacked rows of its settled RANGED matches: (A (2 n, 3), blocks [n x (2, 2)], nu (2 n,), kappa (n,))."""
        P, B = self.P, len(blobs)
        sx, sy, sh = xhat
        G = pr.noise_jacobian(control, sh)
        Qc = self.Qt[1:, 1:]
        out = [([], [], [], []) for _ in range(P)]
        ar = np.arange(P)
        for b in np.nonzero(~np.isnan(rng))[0]:
            idb = ids[:, b]
            li = np.maximum(idb - 1, 0)
            mean, cov = self.mean[ar, li], self.cov[ar, li]
            settled = (idb > 0) & ~self.potential[ar, li]
            Hx = pose_jacobian(sx, sy, mean)
            Hm = -Hx[..., :2]
            zhat = rref.predicted_measurement(sx, sy, sh, mean)
            nu = np.stack([wrap(blobs[b, 0] - zhat[:, 0]), rng[b] - zhat[:, 1]], axis=-1)
            S2 = Hm @ cov[:, :2, :2] @ np.swapaxes(Hm, -1, -2) + np.diag([self.Qt[0, 0], var[b]])
            A2 = (Hx @ G) * s  # rows s (.) (G' h_x)
            C = cov[:, 2:, 2:] + Qc
            dc = blobs[b, 1:] - mean[:, 2:]
            kap = np.linalg.slogdet(C)[1] + np.einsum("pi,pi->p", dc, np.linalg.solve(C, dc[..., None])[..., 0])
            for p in np.nonzero(settled)[0]:
                out[p][0].append(A2[p])
                out[p][1].append(S2[p])
                out[p][2].append(nu[p])
                out[p][3].append(kap[p])
        return out

    def propose(self, control, z, blobs, ranges=None, variances=None, ids=None, fresh=True):
        blobs = np.asarray(blobs, dtype=np.float64).reshape(-1, 4)
        B = len(blobs)
        rng, var = rref._rows(B, ranges, variances)
        ranged = ~np.isnan(rng)
        if not ranged.any():  # no finite range: the bearing-only proposal, call for call
            self.n_rho = np.zeros(self.P, dtype=np.int32)
            return ProposalOracle.propose(self, control, z, blobs, ids=ids, fresh=fresh)
        z = np.asarray(z, dtype=np.float64).reshape(self.P, 3)
        P = self.P
        s = pr.control_sigmas(control)
        x0, y0, h0 = self.x.copy(), self.y.copy(), self.h.copy()
        xhat = pr.move(x0, y0, h0, control, np.zeros((P, 3)))
        # association at the predicted pose, against the untouched landmarks: ranged blobs at their measured points
        self.x, self.y, self.h = xhat
        if ids is None:
            ids = self.associate(blobs, rng, var)
        else:
            ids = np.asarray(ids, dtype=np.int32)
            ids = (ids if ids.ndim == 2 else np.broadcast_to(ids.reshape(1, B), (P, B))).copy()
        plain = self.matches(xhat, control, s, blobs, np.where(ranged[None, :], 0, ids))  # the unranged matches: ProposalOracle's rows
        both = self.ranged_rows(xhat, control, s, blobs, rng, var, ids)
        self.xi, self.dlogw, self.used = np.empty((P, 3)), np.empty(P), np.empty(P, dtype=np.int32)
        self.n_rho = np.empty(P, dtype=np.int32)
        self.Lambda = np.empty((P, 3, 3))
        for p in range(P):
            A1, D1, nu1, kap1, _ = plain[p]
            A2, S2, nu2, kap2 = both[p]
            n1, n2 = len(nu1), len(nu2)
            A = np.concatenate([A1.reshape(-1, 3)] + [a.reshape(2, 3) for a in A2], axis=0)
            blocks = [np.array([[d]]) for d in D1] + list(S2)
            nu = np.concatenate([np.asarray(nu1, dtype=np.float64)] + [np.asarray(v) for v in nu2])
            kap = np.concatenate([np.asarray(kap1, dtype=np.float64), np.asarray(kap2, dtype=np.float64)])
            low = B - n1 - n2
            if n1 + n2:
                DiA = np.linalg.solve(block_diagonal(blocks), A)
                Lam = np.identity(3) + A.T @ DiA
                eta = DiA.T @ nu
                R = np.linalg.cholesky(Lam)
                self.xi[p] = np.linalg.solve(Lam, eta) + np.linalg.solve(R.T, z[p])
            else:
                Lam = np.identity(3)
                self.xi[p] = z[p]
            self.Lambda[p] = Lam
            self.dlogw[p] = delta_dense_blocks(A, blocks, nu, kap, low)
            self.used[p] = n1 + n2
            self.n_rho[p] = n2
        self.xhat = np.stack(xhat, axis=1)
        self.ids = ids
        # the move, with the normals xi; the range-bearing update at the sampled pose with the settled ids; the weight from the proposal
        self.x, self.y, self.h = pr.move(x0, y0, h0, control, s * self.xi)
        logw0 = np.zeros(P) if fresh else self.logw.copy()
        self.observe(blobs, ids, rng, var)
        self.logw = logw0 + self.dlogw
        return ids

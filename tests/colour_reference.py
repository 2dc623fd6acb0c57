"""The colour table's reference (a helper: not a test, not a conftest).

The colour block of a landmark takes C' = C - C (C + Qc)^-1 C at every update, which is the information-form update
C'^-1 = C^-1 + Qc^-1.  Hence level k of the sequence is

    C_k = (C_0^-1 + k Qc^-1)^-1

with no iteration.  Every float64 is an exact rational, so the formula is evaluated in fractions.Fraction: there is no precision
to choose, and it shares no form with the kernels (C - C M, Qc M) or with the oracle ((I - K H) Sigma behind a 4x4 LU).

`e_ref` is the yardstick's other half: how far the oracle's own float64 arithmetic lands from the exact level.  The GPU tests
bound the device's error by a multiple of it (BOUND), so the bound follows the conditioning of the world, not the device."""
from fractions import Fraction

import numpy as np

from oracle.fastslam_oracle import ekf_update_dense

ULP = 2.0 ** -52
FULL_QT = np.zeros((4, 4))  # test_gpu_colour_table.FULL_QT (held equal by the CPU file)
FULL_QT[0, 0] = 0.1
FULL_QT[1:, 1:] = np.array([[0.12, 0.02, -0.01], [0.02, 0.1, 0.015], [-0.01, 0.015, 0.09]])
FACTOR, FLOOR_ULPS = 4, 64  # rel_err(device) <= FACTOR * e_ref(k) + FLOOR_ULPS * 2^-52


def to_fractions(M):
    M = np.asarray(M, dtype=np.float64)
    return [[Fraction(float(M[i, j])) for j in range(3)] for i in range(3)]


def _inv3(A):
    """Inverse of a 3x3 of Fractions: adjugate over determinant, exact."""
    (a, b, c), (d, e, f), (g, h, i) = A
    co = [[e * i - f * h, c * h - b * i, b * f - c * e],
          [f * g - d * i, a * i - c * g, c * d - a * f],
          [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    if det == 0:
        raise ZeroDivisionError("singular 3x3")
    return [[co[r][s] / det for s in range(3)] for r in range(3)]


def _mul3(A, B):
    return [[sum(A[r][t] * B[t][s] for t in range(3)) for s in range(3)] for r in range(3)]


def _rounded(F):
    return np.array([[float(F[r][s]) for s in range(3)] for r in range(3)])  # Fraction.__float__ rounds correctly


def exact_level(C0, Qc, k):
    """(3x3 of Fractions, its correctly rounded float64) of (C0^-1 + k Qc^-1)^-1."""
    C0f, Qcf = to_fractions(C0), to_fractions(Qc)
    if k == 0:
        return C0f, _rounded(C0f)
    Ci, Qi = _inv3(C0f), _inv3(Qcf)
    F = _inv3([[Ci[r][s] + k * Qi[r][s] for s in range(3)] for r in range(3)])
    return F, _rounded(F)


def exact_levels_iterated(C0, Qc, n):
    """Levels 0 .. n by the recurrence C' = C - C (C + Qc)^-1 C itself, in Fractions (the closed form's own check)."""
    C, Qcf = to_fractions(C0), to_fractions(Qc)
    out = [C]
    for _ in range(n):
        S = _inv3([[C[r][s] + Qcf[r][s] for s in range(3)] for r in range(3)])
        CSC = _mul3(_mul3(C, S), C)
        C = [[C[r][s] - CSC[r][s] for s in range(3)] for r in range(3)]
        out.append(C)
    return out


def ref64_levels(mean, cov5, Qt, pose, blob, n):
    """The colour block after each of n updates by oracle.fastslam_oracle.ekf_update_dense -- the reference's float64 arithmetic,
    (I - K H) Sigma with a 4x4 np.linalg.inv -- batched over leading dimensions of mean / cov5 / blob.  Returns (n, ..., 3, 3)."""
    mean = np.array(mean, dtype=np.float64)
    cov = np.array(cov5, dtype=np.float64)
    Qt = np.asarray(Qt, dtype=np.float64).reshape(4, 4)
    out = []
    for _ in range(n):
        mean, cov, _, _ = ekf_update_dense(pose[0], pose[1], mean, cov, blob, Qt)
        out.append(cov[..., 2:, 2:].copy())
    return np.array(out)


def rel_err(C, exact):
    """max |C - exact| / max |exact| over the block, the difference taken in Fractions."""
    Cf = to_fractions(C)
    num = max(abs(Cf[r][s] - exact[r][s]) for r in range(3) for s in range(3))
    den = max(abs(exact[r][s]) for r in range(3) for s in range(3))
    return float(num / den)


def bound(e_ref_k):
    return FACTOR * e_ref_k + FLOOR_ULPS * ULP


_E_REF = {}


def e_ref(key, means, covs, Qt, seen, levels):
    """{level: worst rel_err of ref64_levels against exact_level over the landmarks `seen`} with exact blobs from the origin, the
    blocks' smallest eigenvalue along the way, and the exact levels themselves ({(landmark, level): Fractions}).  Computed once per
    `key` (the caller names its world) and shared: nobody may change what comes back."""
    if key in _E_REF:
        return _E_REF[key]
    seen = np.asarray(seen)
    Qt = np.asarray(Qt, dtype=np.float64).reshape(4, 4)
    blobs = np.empty((len(seen), 4))
    blobs[:, 0] = np.arctan2(means[seen, 1], means[seen, 0])
    blobs[:, 1:] = means[seen, 2:]
    ref = ref64_levels(means[seen], covs[seen], Qt, (0.0, 0.0), blobs, max(levels))
    worst, exact, min_eig = {}, {}, np.inf
    for k in levels:
        w = 0.0
        for i, l in enumerate(seen):
            F, _ = exact_level(covs[l, 2:, 2:], Qt[1:, 1:], k)
            exact[(int(l), k)] = F
            blk = ref[k - 1, i] if k > 0 else covs[l, 2:, 2:]
            w = max(w, rel_err(blk, F))
            min_eig = min(min_eig, float(np.linalg.eigvalsh(0.5 * (blk + blk.T)).min()))
        worst[k] = w
    _E_REF[key] = (worst, min_eig, exact)
    return _E_REF[key]


# ---- the worlds of the deep-level tests (CPU: the reference's drift; GPU: the device against the exact levels)
DEEP_LEVELS = (1, 2, 3, 8, 9, 64, 300)  # downloads of the 300-scan run
SHALLOW_LEVELS = (8, 9, 16, 40)         # ... of the 40-scan run on a table of eight levels
DEEP_WORLDS = ("W1", "W2", "W3", "W4")
DEEP_SIZES = (520, 1030)                # NP = 1 and NP = 2 instances of k_step_pub


def world_at(L, seed=11, one_block=True):
    """test_gpu_colour_table.world at any map size: the same draws in the same order (that module's L is a global of its own;
    tests/test_colour_recurrence_reference.py holds the two equal at L = 520)."""
    rs = np.random.RandomState(seed)
    phi = -np.pi + 2 * np.pi * np.arange(L) / float(L) + 0.01
    rho = rs.uniform(8.0, 30.0, size=L)
    means = np.empty((L, 5))
    means[:, 0] = rho * np.cos(phi)
    means[:, 1] = rho * np.sin(phi)
    means[:, 2:] = rs.uniform(0.0, 255.0, size=(L, 3))
    covs = np.broadcast_to(0.25 * np.identity(5), (L, 5, 5)).copy()
    if not one_block:
        for l in range(L):
            a = rs.uniform(-0.3, 0.3, size=(3, 3))
            covs[l, 2:, 2:] = 0.2 * np.identity(3) + a @ a.T
    return means, covs


def seen_of(L, B=64):
    return np.arange(3, L, 8)[:B]


def deep_world(name, L):
    """(means, covs, Qt 4x4, immutable, seen).  W1: one colour block, the default Qt (diagonal: C' = Qc M).  W2: a block per
    landmark, a full Qc (C' = C - C M).  W3: W2 with the blocks x 1200 and Qc x 0.1, |C| / |Qc| about 3e4: the subtraction
    loses four to five digits at the first levels.  W4: W2's blocks under a diagonal Qc with unequal entries, 0.1, 0.02 and 3: the short
    form C' = Qc M with a row factor of its own per row (under W1's Qt = 0.1 I the three are one number)."""
    if name == "W1":
        means, covs = world_at(L)
        Qt = 0.1 * np.identity(4)
    elif name == "W4":
        means, covs = world_at(L, seed=12, one_block=False)
        Qt = np.diag([0.1, 0.1, 0.02, 3.0])
    else:
        means, covs = world_at(L, seed=12, one_block=False)
        Qt = FULL_QT.copy()
        if name == "W3":
            covs[:, 2:, 2:] *= 1200.0
            Qt[1:, 1:] *= 0.1
    seen = seen_of(L)
    imm = np.zeros(L, dtype=np.uint8)
    imm[seen[5]] = imm[seen[40]] = 1
    return means, covs, Qt, imm, seen


def deep_e_ref(name, L):
    means, covs, Qt, imm, seen = deep_world(name, L)
    return e_ref(("deep", name, L), means, covs, Qt, seen, sorted(set(DEEP_LEVELS + SHALLOW_LEVELS)))

"""CPU: the colour table's reference (tests/colour_reference.py).

The closed form C_k = (C_0^-1 + k Qc^-1)^-1 is held to the recurrence C' = C - C (C + Qc)^-1 C itself, both in exact rational
arithmetic, and the oracle's float64 update is measured against it: e_ref(k), the figure the GPU tests' bound is made of
(tests/test_gpu_colour_table_reference.py).  e_ref is recorded (run with -s to see it), not judged: the oracle restates the
reference's arithmetic, and what that arithmetic loses is a property of the world."""
from fractions import Fraction

import numpy as np
import pytest

import colour_reference as cr
from test_gpu_colour_table import FULL_QT


def _spd(seed):
    rs = np.random.RandomState(seed)
    a = rs.normal(size=(3, 3))
    return a @ a.T + 0.1 * np.identity(3)


CASES = {
    "scalar_identity": (0.25 * np.identity(3), 0.1 * np.identity(3)),
    "random_spd": (_spd(1), _spd(2)),
    "diagonal_qc_unequal": (_spd(3), np.diag([0.1, 0.02, 3.0])),
    "full_qc": (_spd(4), FULL_QT[1:, 1:].copy()),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_equals_the_iterated_recurrence(name):
    C0, Qc = CASES[name]
    it = cr.exact_levels_iterated(C0, Qc, 12)
    assert len(it) == 13
    for k in range(13):
        F, r = cr.exact_level(C0, Qc, k)
        assert F == it[k], (name, k)  # Fractions: equal means equal
        assert all(isinstance(F[i][j], Fraction) for i in range(3) for j in range(3))
        assert r.shape == (3, 3) and r.dtype == np.float64 and cr.rel_err(r, F) <= 2.0 ** -53  # correctly rounded
    assert np.array_equal(cr.exact_level(C0, Qc, 0)[1], C0)
    # the levels shrink: C_k - C_(k+1) is positive definite
    for k in range(12):
        d = np.array([[float(it[k][i][j] - it[k + 1][i][j]) for j in range(3)] for i in range(3)])
        assert np.linalg.eigvalsh(d).min() > 0


def test_the_helper_restates_the_twin_file_world():
    import test_gpu_colour_table as tct

    assert tct.L == 520 and np.array_equal(cr.FULL_QT, tct.FULL_QT) and np.array_equal(cr.seen_of(520), tct.SEEN)
    for seed, one_block in ((11, True), (12, False)):
        for x, y in zip(cr.world_at(520, seed=seed, one_block=one_block), tct.world(seed=seed, one_block=one_block)):
            assert np.array_equal(x, y)


def test_rel_err_takes_the_difference_exactly():
    F, r = cr.exact_level(_spd(5), _spd(6), 3)
    assert cr.rel_err(r, cr.to_fractions(r)) == 0.0
    big = max(abs(float(F[i][j])) for i in range(3) for j in range(3))
    bumped = r.copy()
    bumped[1, 2] = np.nextafter(bumped[1, 2], np.inf)  # one ulp of one entry: seen, and about the size it should be
    e = cr.rel_err(bumped, F)
    assert 0.0 < e <= 1.5 * np.spacing(abs(r[1, 2])) / big + 2.0 ** -53


def test_ref64_levels_is_the_oracle_filter_step_by_step():
    """ref64_levels restates nothing: it is ekf_update_dense, and the block it returns is what OracleFilter.observe leaves."""
    from oracle.fastslam_oracle import OracleFilter

    means, covs, Qt, imm, seen = cr.deep_world("W2", 520)
    seen = seen[:4]
    blobs = np.empty((4, 4))
    blobs[:, 0] = np.arctan2(means[seen, 1], means[seen, 0])
    blobs[:, 1:] = means[seen, 2:]
    lv = cr.ref64_levels(means[seen], covs[seen], Qt, (0.0, 0.0), blobs, 3)
    o = OracleFilter(1, means, covs)
    o.Qt = Qt.copy()
    for s in range(3):
        o.observe(blobs, ids=seen + 1)
        assert np.array_equal(o.cov[0, seen][:, 2:, 2:], lv[s])


@pytest.mark.parametrize("L", cr.DEEP_SIZES)
@pytest.mark.parametrize("name", cr.DEEP_WORLDS)
def test_reference_drift_is_recorded(name, L):
    worst, min_eig, exact = cr.deep_e_ref(name, L)
    levels = sorted(worst)
    assert levels == sorted(set(cr.DEEP_LEVELS + cr.SHALLOW_LEVELS))
    print("\ne_ref %s L=%d: " % (name, L) + "  ".join("k=%d %.3g (%.0f ulp)" % (k, worst[k], worst[k] / cr.ULP) for k in levels))
    assert all(np.isfinite(worst[k]) for k in levels)
    assert min_eig > 0  # the reference's blocks stay positive definite

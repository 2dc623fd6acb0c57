"""GPU: the colour table (pk_colour_table_stats).  While every map descends from one pk_upload_map the colour
covariance of a landmark is a function of (landmark, update count), and the 512-lane publish / subscribe kernel takes it from a
shared table instead of streaming six rows per landmark through every slot.  Nothing anybody can see may change: every test runs
two filters side by side -- `colour_table` = 0 and the default -- and compares poses, log-weights and downloaded landmarks (means,
covariances, counts) with np.array_equal.  Each test also asserts, through the statistics, that the mode really took the scans it
claims: a run that silently fell back would prove nothing.

The world is restated here: L = 520 landmarks on a ring (the 512 < L <= 2048 route), P = 96 particles, scans of B = 64 blobs."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, P, B = 520, 96, 64
LOG = 1  # PK_WEIGHTS_LOG


def world(seed=11, one_block=True):
    rs = np.random.RandomState(seed)
    phi = -math.pi + 2 * math.pi * np.arange(L) / float(L) + 0.01
    rho = rs.uniform(8.0, 30.0, size=L)
    means = np.empty((L, 5))
    means[:, 0] = rho * np.cos(phi)
    means[:, 1] = rho * np.sin(phi)
    means[:, 2:] = rs.uniform(0.0, 255.0, size=(L, 3))
    covs = np.broadcast_to(0.25 * np.identity(5), (L, 5, 5)).copy()
    if not one_block:  # a different symmetric positive definite colour block per landmark
        for l in range(L):
            a = rs.uniform(-0.3, 0.3, size=(3, 3))
            covs[l, 2:, 2:] = 0.2 * np.identity(3) + a @ a.T
    return means, covs


def scan_of(means, pose, seen):
    x, y, h = pose
    blobs = np.empty((len(seen), 4))
    blobs[:, 0] = np.arctan2(means[seen, 1] - y, means[seen, 0] - x) - h
    blobs[:, 1:] = means[seen, 2:]
    return blobs


def truth(n, v=0.2, w=0.05, dt=0.1):
    poses, (x, y, h) = [], (0.0, 0.0, 0.0)
    for _ in range(n):
        h1 = h + w * dt / 2
        x, y, h = x + v * dt * math.cos(h1), y + v * dt * math.sin(h1), h1 + w * dt / 2
        poses.append((x, y, h))
    return poses


SEEN = np.arange(3, L, 8)[:B]  # the landmarks a scan sees: every eighth, the same in every scan (their counts climb step by step)


def pair(lib, means, covs, immutable=None, Qt=None, opts=None):
    out = []
    for table in (0, None):
        f = lib.DeviceFilter(P, L)
        if table is not None:
            f.set_option("colour_table", table)
        for k, v in (opts or {}).items():
            f.set_option(k, v)
        if Qt is not None:
            f.set_measurement_noise(Qt)
        f.upload_map(means, covs.reshape(L, 25), immutable)
        poses = np.zeros((P, 4))
        poses[:, 3] = 1.0
        f.upload_poses(poses)
        out.append(f)
    return out


def step(fs, s, blobs, us):
    for f in fs:
        f.step(0.2, 0.05, 0.1, blobs, us[s], seed=5, draw=s, domain=LOG)


def same_poses(fs):
    a, b = fs
    assert np.array_equal(a.download_poses(), b.download_poses())
    assert np.array_equal(a.download_log_weights(), b.download_log_weights())


def same_maps(fs):
    a, b = fs
    for x, y in zip(a.download_landmarks(), b.download_landmarks()):
        assert np.array_equal(x, y)


def us_of(n):
    return np.random.RandomState(99).uniform(size=n)


def close(fs):
    for f in fs:
        f.close()


def test_six_steps_with_resampling_one_colour_block(lib):
    means, covs = world()
    fs = pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        step(fs, s, scan_of(means, tr[s], SEEN), us)
        same_poses(fs)
        assert fs[1].observe_route() == "ml_regs" and fs[1].observe_published() and fs[1].observe_flagged()[0] == 0
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 6 and st["materialisations"] == 0 and st["depth"] == 1024
    assert fs[0].colour_table_stats()["scans"] == 0
    assert fs[1].observe_bytes(B)[1] < fs[0].observe_bytes(B)[1]  # 136 against 232 bytes per particle.landmark
    same_maps(fs)
    assert fs[1].colour_table_stats()["materialisations"] == 1
    m, c, k = fs[1].download_landmarks()
    assert k.max() == 12 and (k[:, SEEN] > 0).all()  # six scans, an update each
    close(fs)


def test_blocks_per_landmark_immutables_full_qt_and_a_landmark_with_two_blobs(lib):
    means, covs = world(seed=12, one_block=False)
    imm = np.zeros(L, dtype=np.uint8)
    imm[SEEN[5]] = imm[SEEN[40]] = 1
    Qt = np.zeros((4, 4))
    Qt[0, 0] = 0.1
    Qt[1:, 1:] = np.array([[0.12, 0.02, -0.01], [0.02, 0.1, 0.015], [-0.01, 0.015, 0.09]])
    fs = pair(lib, means, covs, imm, Qt.reshape(16))
    us, tr = us_of(6), truth(6)
    twice = SEEN[20]
    for s in range(6):
        blobs = scan_of(means, tr[s], SEEN)
        if s == 2:  # one landmark is seen twice in this scan: two updates, count += 4
            extra = scan_of(means, tr[s], np.array([twice]))
            extra[0, 0] += 1e-3
            extra[0, 1:] += (0.05, -0.05, 0.02)
            blobs = np.vstack([blobs[:-1], extra])
        step(fs, s, blobs, us)
        same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 6
    same_maps(fs)
    m, c, k = fs[1].download_landmarks()
    assert k[:, twice].max() == 14                                    # six scans, one of them twice
    assert (k[:, SEEN[5]] == 0).all() and (k[:, SEEN[40]] == 0).all()  # immutable: never off their level
    assert np.array_equal(c[:, SEEN[5]], np.broadcast_to(covs[SEEN[5]], (P, 5, 5)))
    close(fs)


def test_scans_that_go_to_the_general_kernels(lib):
    means, covs = world(seed=13)
    # look-alike neighbours (contested blobs: the publish table has entries)
    means[SEEN + 1, 2:] = means[SEEN, 2:] + 2.0
    fs = pair(lib, means, covs)
    us, tr = us_of(5), truth(5)
    flagged = []
    for s in range(5):
        blobs = scan_of(means, tr[s], SEEN)
        if s == 1:  # more than four look-alike blobs on one landmark: its particles are handed on
            j = SEEN[10]
            extra = np.repeat(scan_of(means, tr[s], np.array([j])), 6, axis=0)
            extra[:, 0] += 1e-3 * np.arange(1, 7)
            extra[:, 1] += 0.03 * np.arange(1, 7)
            blobs = np.vstack([blobs[:-6], extra])
        for f in fs:
            f.set_option("pub_entry_limit", 1 if s == 3 else 0)  # s == 3: the table "does not fit", the kernel stands back
        step(fs, s, blobs, us)
        same_poses(fs)
        flagged.append(fs[1].observe_flagged()[0])
        assert fs[0].observe_flagged()[0] == flagged[-1]
    assert flagged[1] > 0 and flagged[3] == P and flagged[0] == flagged[2] == flagged[4] == 0
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 5 and st["materialisations"] == 0
    same_maps(fs)
    close(fs)


def test_a_download_in_mid_run_materialises_and_the_mode_goes_on(lib):
    means, covs = world(seed=14)
    fs = pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        step(fs, s, scan_of(means, tr[s], SEEN), us)
        if s == 2:
            same_maps(fs)
            st = fs[1].colour_table_stats()
            assert st["engaged"] == 1 and st["scans"] == 3 and st["materialisations"] == 1
            same_maps(fs)  # (the rows are valid now: nothing more to write)
            assert fs[1].colour_table_stats()["materialisations"] == 1
    same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 1 and st["scans"] == 6 and st["materialisations"] == 1
    same_maps(fs)
    assert fs[1].colour_table_stats()["materialisations"] == 2
    close(fs)


def _end_by_upload(f, means):
    m, c, k = f.download_landmarks(7, 8)
    m[0, SEEN[3], 2] += 0.5
    f.upload_landmarks(7, 8, means=m, covs=c.reshape(1, L, 25), counts=k)


def _end_by_noise(f, means):
    Qt = 0.1 * np.identity(4)
    Qt[2, 2] = 0.2
    f.set_measurement_noise(Qt.reshape(16))


def _end_by_grow(f, means):
    f.grow_enable(L - 4, reading_capacity=16)


@pytest.mark.parametrize("ender", [_end_by_upload, _end_by_noise, _end_by_grow])
def test_calls_that_end_the_mode(lib, ender):
    means, covs = world(seed=15)
    fs = pair(lib, means, covs)
    us, tr = us_of(6), truth(6)
    for s in range(6):
        if s == 3:
            assert fs[1].colour_table_stats()["engaged"] == 1 and fs[1].colour_table_stats()["scans"] == 3
            for f in fs:
                ender(f, means)
            assert fs[1].colour_table_stats()["engaged"] == 0
        step(fs, s, scan_of(means, tr[s], SEEN), us)
        same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["engaged"] == 0 and st["scans"] == 3  # off until the next pk_upload_map
    same_maps(fs)
    close(fs)


def test_a_table_of_eight_levels_is_exhausted_and_the_mode_ends(lib):
    means, covs = world(seed=16)
    us, tr = us_of(12), truth(12)
    # step by step (the host knows every scan's levels before the next): it leaves the mode short of the table's end
    fs = pair(lib, means, covs, opts={"colour_table_depth": 8})
    for s in range(12):
        step(fs, s, scan_of(means, tr[s], SEEN), us)
        same_poses(fs)
    st = fs[1].colour_table_stats()
    assert st["depth"] == 8 and st["engaged"] == 0 and 4 <= st["scans"] < 12
    same_maps(fs)
    close(fs)


FULL_QT = np.zeros((4, 4))
FULL_QT[0, 0] = 0.1
FULL_QT[1:, 1:] = np.array([[0.12, 0.02, -0.01], [0.02, 0.1, 0.015], [-0.01, 0.015, 0.09]])


@pytest.mark.parametrize("full_qt", [False, True])
def test_levels_beyond_the_table_come_from_the_recurrence(lib, full_qt):
    """`colour_table_margin` = 0: the host never leaves the mode for the table's end, so from the ninth scan on every seen landmark
    sits on a level the table of eight does not hold -- in k_step_pub, in k_candidates (the reference particle), in k_colour_rows
    over handed-on particles, over one downloaded particle and over the whole buffer."""
    means, covs = world(seed=17, one_block=not full_qt)
    means[SEEN + 1, 2:] = means[SEEN, 2:] + 2.0  # look-alike neighbours, as in the scans that go to the general kernels
    fs = pair(lib, means, covs, Qt=FULL_QT.reshape(16) if full_qt else None, opts={"colour_table_depth": 8, "colour_table_margin": 0})
    us, tr = us_of(12), truth(12)
    for s in range(12):
        blobs = scan_of(means, tr[s], SEEN)
        if s == 10:  # more than four look-alike blobs on one landmark: its particles are handed on, levels 10 and up in their slots
            extra = np.repeat(scan_of(means, tr[s], np.array([SEEN[10]])), 6, axis=0)
            extra[:, 0] += 1e-3 * np.arange(1, 7)
            extra[:, 1] += 0.03 * np.arange(1, 7)
            blobs = np.vstack([blobs[:-6], extra])
        step(fs, s, blobs, us)
        same_poses(fs)
        if s == 10:
            assert fs[1].observe_flagged()[0] > 0 and fs[0].observe_flagged()[0] == fs[1].observe_flagged()[0]
        if s == 8:  # one particle's map: its slots alone are written, the buffer stays stale
            for x, y in zip(fs[0].download_landmarks(7, 8), fs[1].download_landmarks(7, 8)):
                assert np.array_equal(x, y)
            assert fs[1].colour_table_stats()["materialisations"] == 0
        if s == 9:  # the whole buffer, levels 9 and 10 in it
            same_maps(fs)
            assert fs[1].colour_table_stats()["materialisations"] == 1
            assert fs[1].download_landmarks()[2].max() // 2 > 8  # (beyond the table's last level, 7)
    st = fs[1].colour_table_stats()
    assert st["depth"] == 8 and st["engaged"] == 1 and st["scans"] == 12
    same_maps(fs)
    k = fs[1].download_landmarks()[2]
    assert k.max() // 2 >= 12 > st["depth"]  # twelve updates on a table of eight levels
    close(fs)

"""What the estimate of the discovered landmarks costs (pk_map_discovered, pk_k_mapmatch.hip) on one GPU.  One JSON line each:
  1. on a grown filter of 10 000 x (40 + 6) and of 100 000 x (2 000 + 16): ms per call from the handle's PK_T_SUMMARY hipEvents over
     20 calls behind one untimed call, uniform and by the weights, the host's wall clock per call beside it; pk_map_summary on the
     same filter in the same process; and the wall clock of one filter step (motion, observe, resample) of that shape;
  2. at 10 000 only, the host route it replaces: download_landmarks + grow_download of all particles, then the NumPy reference of
     the tests (tests/map_match_reference.py), host wall clock.
    python scripts/gpu_map_discovered_cost.py [--out FILE] [--small-only]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from parakeet_slam_amd import _lib  # noqa: E402

CALLS = 20
SUMMARY_BIT = 1 << _lib.PK_T_NAMES.index("summary")
RADIUS, COLOUR_RADIUS = 3.0, 30.0
EMPTY_COLOUR = 2.0 ** 100  # colour of a spare slot that holds nothing yet (FastSLAM.EMPTY_COLOUR)


def ring_world(L, seed=123):
    rs = np.random.RandomState(seed)
    phi = -np.pi + 2 * np.pi * np.arange(L) / float(L) + 0.01
    rho = rs.uniform(8.0, 30.0, size=L)
    m = np.empty((L, 5))
    m[:, 0], m[:, 1] = rho * np.cos(phi), rho * np.sin(phi)
    m[:, 2:] = rs.uniform(0.0, 255.0, size=(L, 3))
    return m


def scan(world, pose, seen):
    x, y, h = pose
    b = np.empty((len(seen), 4))
    b[:, 0] = np.arctan2(world[seen, 1] - y, world[seen, 0] - x) - h
    b[:, 1:] = world[seen, 2:]
    return b


def grown_filter(P, L0, U, S, steps=6, B=64):
    """P x (L0 + S): L0 preset landmarks, U unknown ones in every scan beside up to B of the preset ones."""
    world = ring_world(L0 + U)
    L = L0 + S
    means = np.zeros((L, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    covs = np.tile(np.identity(5).reshape(25), (L, 1))
    covs[:L0] = (0.25 * np.identity(5)).reshape(25)
    f = _lib.DeviceFilter(P, L)
    f.upload_map(means, covs)
    f.grow_enable(L0, 64, 30.0)
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0
    f.upload_poses(poses)
    seen = np.concatenate([np.arange(0, L0, max(1, L0 // B))[:B], np.arange(L0, L0 + U)])
    rs = np.random.RandomState(7)
    pose, v, w, dt = (0.0, 0.0, 0.0), 0.8, 0.35, 0.5
    step_ms = []
    for s in range(steps):
        h1 = pose[2] + w * dt / 2
        pose = (pose[0] + v * dt * np.cos(h1), pose[1] + v * dt * np.sin(h1), h1 + w * dt / 2)
        f.synchronize()
        t0 = time.perf_counter()
        f.motion(v, w, dt, seed=5, draw=s)
        f.observe(scan(world, pose, seen), fresh=True)
        f.resample(float(rs.uniform()), domain=_lib.PK_WEIGHTS_LOG)
        f.synchronize()
        step_ms.append((time.perf_counter() - t0) * 1e3)
    return f, float(np.median(step_ms[1:]))


def timed(f, call):
    call()  # (untimed: the scratch is allocated here)
    f.enable_timing(SUMMARY_BIT)
    f.reset_timings()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        call()
    wall = (time.perf_counter() - t0) * 1e3 / CALLS
    ms, n = f.timings()["summary"]
    f.enable_timing(False)
    assert n == CALLS, n
    return ms / n, wall


def estimate_lines(P, L0, U, S):
    f, step_ms = grown_filter(P, L0, U, S)
    used = f.grow_download(readings=False, slot_ids=False)[0][:, 1]
    out = []
    for name, code in (("uniform", _lib.PK_MAP_UNIFORM), ("weights", _lib.PK_MAP_WEIGHTED)):
        ms, wall = timed(f, lambda: f.map_discovered(RADIUS, COLOUR_RADIUS, code))
        d = f.map_discovered(RADIUS, COLOUR_RADIUS, code)
        out.append(dict(what="map_discovered", particles=P, preset_landmarks=L0, spare_slots=S, weighting=name, device_ms_per_call=round(ms, 4),
                        host_wall_ms_per_call=round(wall, 4), step_wall_ms=round(step_ms, 3), spare_slots_in_use_mean=round(float(used.mean()), 2),
                        distinct_slots=int(len(np.unique(f.download_sources()))), reference_features=int(d.mean.shape[0]),
                        support=[round(float(x), 4) for x in d.support], device_bytes=f.device_bytes()))
    ms, wall = timed(f, lambda: f.map_summary())
    out.append(dict(what="map_summary", particles=P, landmarks=L0 + S, device_ms_per_call=round(ms, 4), host_wall_ms_per_call=round(wall, 4)))
    return f, out


def host_route(f):
    """What a caller had to do before: every particle's landmarks and counters to the host, the match and the moments in NumPy."""
    from map_match_reference import reference

    best = f.best_particle()[0]
    t0 = time.perf_counter()
    m, c, k = f.download_landmarks()
    counters = f.grow_download(readings=False, slot_ids=False)[0]
    t1 = time.perf_counter()
    L0 = f.grow_shape()[0]
    u = int(counters[best, 1])
    r = reference(m, c, k, counters[:, 1], L0, m[best, L0:L0 + u], RADIUS, COLOUR_RADIUS)
    t2 = time.perf_counter()
    return dict(what="download_landmarks + grow_download + NumPy", particles=f.P, landmarks=f.L, download_ms=round((t1 - t0) * 1e3, 1),
                reduce_ms=round((t2 - t1) * 1e3, 1), total_ms=round((t2 - t0) * 1e3, 1), host_bytes=int(m.nbytes + c.nbytes + k.nbytes),
                support=[round(float(x), 4) for x in r.support])


if __name__ == "__main__":
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "map_discovered_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)
        return ln

    f, est = estimate_lines(10000, 40, 6, 6)
    for e in est:
        emit(e)
    old = emit(host_route(f))
    emit(dict(what="ratio at 10 000 x (40 + 6)", old_total_ms=old["total_ms"], new_host_wall_ms=est[0]["host_wall_ms_per_call"],
              old_over_new=round(old["total_ms"] / est[0]["host_wall_ms_per_call"], 1)))
    f.close()
    if "--small-only" not in sys.argv:
        f, est = estimate_lines(100000, 2000, 6, 16)
        for e in est:
            emit(e)
        f.close()
    fh.close()

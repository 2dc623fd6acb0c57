"""The map estimate's speed (pk_map_summary, pk_k_mapsum.hip) on one GPU.  One call records, one JSON line each:
  1. the estimate at 10 000 x 500 and at 100 000 x 2 000, behind a resample (runs of equal src) and behind an observe (identity src):
     ms per call from the handle's PK_T_SUMMARY hipEvents, warmed up, over 20 calls -- and the host's wall clock per call beside it
     (the call also copies 2 + 30 L doubles back and finishes them on the host);
  2. at 10 000 x 500, what a caller had to do before for the same numbers: download_landmarks of all particles, then the NumPy
     reduction (host wall clock);
  3. the bytes the kernel must read (distinct slots x slot_bytes) over its time, as a share of the 8 TB/s HBM peak;
  4. the box's device-to-device copy rate (read + write bytes over hipEvent time), measured in the same call.
    python scripts/gpu_map_summary_speed.py [--out FILE] [--small-only]"""
import json
import os
import sys
import time

import numpy as np
import torch  # (plumbing: the copy-rate probe; before the library, so that both share one HIP runtime)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from parakeet_slam_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
CALLS, WARM = 20, 3
SUMMARY_BIT = 1 << _lib.PK_T_NAMES.index("summary")


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


def slot_bytes(L):
    Lp = max((L + 15) & ~15, 16)
    return (14 * Lp * 8 + Lp * 4 + 255) & ~255


def timed(f, weighting):
    for _ in range(WARM):
        f.map_summary(weighting)
    f.enable_timing(SUMMARY_BIT)
    f.reset_timings()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        f.map_summary(weighting)
    wall = (time.perf_counter() - t0) * 1e3 / CALLS
    ms, n = f.timings()["summary"]
    f.enable_timing(False)
    assert n == CALLS, n
    return ms / n, wall


def estimate_lines(P, L, B=64, steps=3):
    world = ring_world(L)
    f = _lib.DeviceFilter(P, L)
    f.upload_map(world, np.tile(0.25 * np.identity(5), (L, 1, 1)).reshape(L, 25))
    poses = np.zeros((P, 4))
    poses[:, 3] = 1.0
    f.upload_poses(poses)
    seen = np.arange(3, L, max(1, L // B))[:B]
    pose, us = (0.0, 0.0, 0.0), np.random.RandomState(7).uniform(size=steps)
    v, w, dt = 0.8, 0.35, 0.5  # (steps long enough for the motion noise to tell the particles apart: the resample then has something to do)
    for s in range(steps):
        h1 = pose[2] + w * dt / 2
        pose = (pose[0] + v * dt * np.cos(h1), pose[1] + v * dt * np.sin(h1), h1 + w * dt / 2)
        f.step(v, w, dt, scan(world, pose, seen), us[s], seed=5, draw=s, domain=_lib.PK_WEIGHTS_LOG)
    out = []
    for state in ("behind a resample", "behind an observe"):
        if state == "behind an observe":
            f.motion(v, w, dt, seed=5, draw=steps)
            f.observe(scan(world, pose, seen), fresh=True)
        distinct = int(len(np.unique(f.download_sources())))
        for name, code in (("uniform", _lib.PK_MAP_UNIFORM), ("weights", _lib.PK_MAP_WEIGHTED)):
            ms, wall = timed(f, code)
            must = distinct * slot_bytes(L)
            out.append(dict(what="map_summary", particles=P, landmarks=L, state=state, weighting=name, distinct_slots=distinct,
                            device_ms_per_call=round(ms, 4), host_wall_ms_per_call=round(wall, 4), bytes_to_read=must,
                            read_rate_TBps=round(must / (ms * 1e-3) / 1e12, 3), share_of_hbm_peak=round(must / (ms * 1e-3) / HBM_PEAK, 3),
                            device_bytes=f.device_bytes()))
    return f, out


def old_way(f):
    """download_landmarks of all particles, then the reduction in NumPy: what the same numbers cost without the entry point."""
    t0 = time.perf_counter()
    m, c, k = f.download_landmarks()
    t1 = time.perf_counter()
    mean = m.mean(axis=0)
    d = m - mean
    between = np.einsum("pli,plj->lij", d, d) / m.shape[0]
    within = c.mean(axis=0)
    count = (k & ~_lib.PK_LANDMARK_POTENTIAL).mean(axis=0)
    t2 = time.perf_counter()
    assert np.isfinite(mean).all() and np.isfinite(between).all() and np.isfinite(within).all() and np.isfinite(count).all()
    return dict(what="download_landmarks + NumPy", particles=f.P, landmarks=f.L, download_ms=round((t1 - t0) * 1e3, 1),
                reduce_ms=round((t2 - t1) * 1e3, 1), total_ms=round((t2 - t0) * 1e3, 1), host_bytes=int(m.nbytes + c.nbytes + k.nbytes))


def copy_rate(nbytes=4 << 30, reps=10):
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a.zero_()
    for _ in range(3):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return dict(what="device-to-device copy", bytes=nbytes, ms=round(ms, 4), read_plus_write_TBps=round(2 * nbytes / (ms * 1e-3) / 1e12, 3),
                share_of_hbm_peak=round(2 * nbytes / (ms * 1e-3) / HBM_PEAK, 3))


if __name__ == "__main__":
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "map_summary_speed.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)
        return ln

    emit(copy_rate())
    f, est = estimate_lines(10000, 500)
    for e in est:
        emit(e)
    old = emit(old_way(f))
    new_ms = [e["host_wall_ms_per_call"] for e in est if e["state"] == "behind an observe" and e["weighting"] == "uniform"][0]
    emit(dict(what="ratio at 10 000 x 500", old_total_ms=old["total_ms"], new_host_wall_ms=new_ms, old_over_new=round(old["total_ms"] / new_ms, 1)))
    f.close()
    if "--small-only" not in sys.argv:
        f, est = estimate_lines(100000, 2000)
        for e in est:
            emit(e)
        f.close()
    emit(copy_rate())  # (again at the end: the spread of the probe itself)
    fh.close()

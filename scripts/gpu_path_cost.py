"""What the path estimate costs (pk_path_enable, pk_k_path.hip) on one GPU.  One call, one JSON line per figure:
  1. the headline step (bench.py's workload: 100 000 particles x 2 000 landmarks through pk_step) with recording off and on,
     alternating, five runs each: every run a fresh filter through the same 5 warm-up + 50 timed steps, host wall clock around the
     timed steps with the stream drained -- the comparison is the same build with recording off, and the off-runs' own spread is
     the yardstick;
  2. pk_path_summary at 100 000 particles with 64 and with 1 024 rows held, on a ring whose every lineage survives (uniform weights:
     the most work, every count is non-zero) and on one that coalesces (weights kept from step to step): ms per call from the
     handle's PK_T_SUMMARY hipEvents and the host's wall clock beside it, over five calls;
  3. pk_path_trace of all particles at 64 rows.
    python scripts/gpu_path_cost.py [--out FILE] [--particles P] [--landmarks L]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the headline's inputs)
from parakeet_slam_amd import _lib  # noqa: E402

WARM, STEPS, RUNS, RING = 5, 50, 5, 64
SUMMARY_BIT = 1 << _lib.PK_T_NAMES.index("summary")


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def step_run(P, L, inputs, record):
    means, covs, scans, ws, us = inputs
    f = _lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    if record:
        f.path_enable(RING)

    def one(s):
        f.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, domain=_lib.PK_WEIGHTS_LOG)

    for s in range(WARM):
        one(s)
    f.synchronize()
    t0 = time.perf_counter()
    for s in range(WARM, WARM + STEPS):
        one(s)
    f.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / STEPS
    shape = f.path_shape() if record else None
    summary = f.summary()
    f.close()
    return ms, shape, summary


def summary_cost(P, coalescing, emit):
    rs = np.random.RandomState(3)
    f = _lib.DeviceFilter(P, 0)
    poses = np.zeros((P, 4))
    poses[:, :3] = rs.uniform(-1.0, 1.0, (P, 3))
    poses[:, 3] = rs.uniform(0.5, 1.0, P) if coalescing else 1.0
    f.upload_poses(poses)
    f.path_enable(1024)
    held = 0
    for want in (64, 1024):
        while held < want:
            f.motion(0.2, 0.1, 0.1, seed=11, draw=held)
            f.resample(float(rs.uniform()), domain=_lib.PK_WEIGHTS_LOG)
            held += 1
        f.path_summary()  # (scratch, first touch)
        f.enable_timing(SUMMARY_BIT)
        f.reset_timings()
        t0 = time.perf_counter()
        for _ in range(5):
            got = f.path_summary()
        wall = (time.perf_counter() - t0) * 1e3 / 5
        ms, n = f.timings()["summary"]
        f.enable_timing(False)
        emit(dict(what="pk_path_summary", particles=P, held=held, ring="coalescing" if coalescing else "every lineage survives",
                  device_ms_per_call=round(ms / n, 4), host_wall_ms_per_call=round(wall, 4), launches_per_call=held + 3,
                  survivors_oldest_row=int(got.survivors[0]), survivors_row_held_minus_8=int(got.survivors[held - 8]),
                  device_bytes=f.device_bytes()))
        if held == 64:
            idx = np.arange(P)
            f.path_trace(idx)
            t0 = time.perf_counter()
            f.path_trace(idx)
            emit(dict(what="pk_path_trace, all particles", particles=P, held=held, host_wall_ms=round((time.perf_counter() - t0) * 1e3, 3)))
    f.close()


if __name__ == "__main__":
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "path_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)
        return ln

    P, L = arg("--particles", bench.DEFAULT_P), arg("--landmarks", bench.DEFAULT_L)
    means, covs, scans = bench.synthetic_inputs(L, WARM + STEPS)
    ws = bench.synthetic_controls(WARM + STEPS)
    import random

    rnd = random.Random(7)
    inputs = (means, covs, scans, ws, [rnd.random() for _ in range(WARM + STEPS)])
    step_run(min(P, 4096), L, inputs, True)  # (the process's first launches, code objects loaded: not a figure)
    off, on, summaries = [], [], set()
    for run in range(RUNS):
        for record in (False, True):
            ms, shape, summary = step_run(P, L, inputs, record)
            (on if record else off).append(ms)
            summaries.add(summary)
            emit(dict(what="step", particles=P, landmarks=L, record_path=RING if record else 0, run=run, ms_per_step=round(ms, 4), path_shape=shape))
    spread = (max(off) - min(off)) / np.median(off)
    emit(dict(what="recording off against on", particles=P, landmarks=L, steps=STEPS, runs=RUNS, off_ms=[round(v, 4) for v in off],
              on_ms=[round(v, 4) for v in on], off_median=round(float(np.median(off)), 4), on_median=round(float(np.median(on)), 4),
              on_over_off=round(float(np.median(on) / np.median(off)), 5), off_spread_max_minus_min_over_median=round(float(spread), 5),
              same_summary_in_every_run=len(summaries) == 1))
    for coalescing in (False, True):
        summary_cost(P, coalescing, emit)
    fh.close()

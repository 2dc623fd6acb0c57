"""What adaptive resampling costs and buys (pk_step_adaptive, pk_summary_weighted; pk_k_adaptive.hip) on one GPU.  After
gpu_path_cost.py's method; one call, one JSON line per figure:
  1. the price of the gate: the headline step (bench.py's workload: 100 000 particles x 2 000 landmarks) through pk_step and through
     pk_step_adaptive with a threshold of 2 (always resamples: the same work plus the gate), alternating, five runs each: every run a
     fresh filter through the same 5 warm-up + 50 timed steps, host wall clock around the timed steps with the stream drained -- the
     yardstick is pk_step's own run-to-run spread in the same call;
  2. what it buys: a 10 000 x 500 scene over 64 steps with a ring of 64 rows, at thresholds None (pk_step), 0.5 and 0.25: the
     resamples taken and path_summary().survivors at rows 0, 16, 32, 48 (recorded, not asserted);
  3. the summary call: pk_summary_weighted against pk_summary at 100 000 particles, PK_T_SUMMARY hipEvents over 20 calls.
--four-steps plain|adaptive: nothing but four steps of a 10 000 x 500 filter, for `rocprofv3 --kernel-trace --stats` (a run of its
own, no counters); --lib NAME: another build of the library beside the package's (one from before these entry points existed too).
    python scripts/gpu_adaptive_cost.py [--out FILE] [--particles P] [--landmarks L]"""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the headline's inputs)
from parakeet_slam_amd import _lib  # noqa: E402

WARM, STEPS, RUNS, RING = 5, 50, 5, 64
SUMMARY_BIT = 1 << _lib.PK_T_NAMES.index("summary")
LOG = _lib.PK_WEIGHTS_LOG
ADAPTIVE_SYMBOLS = ("pk_resample_adaptive", "pk_step_adaptive", "pk_resample_stats", "pk_weight_sums", "pk_summary_weighted",
                    "pk_upload_log_weights")


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def inputs_for(L, steps):
    means, covs, scans = bench.synthetic_inputs(L, steps)
    rnd = random.Random(7)
    return means, covs, scans, bench.synthetic_controls(steps), [rnd.random() for _ in range(steps)]


def stepper(f, inputs, theta):
    _, _, scans, ws, us = inputs
    if theta is None:
        return lambda s: f.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, domain=LOG)
    return lambda s: f.step_adaptive(0.2, ws[s], 0.1, scans[s], us[s], theta, seed=7, draw=s, domain=LOG)


def new_filter(P, L, inputs):
    f = _lib.DeviceFilter(P, L)
    f.upload_map(inputs[0], inputs[1].reshape(L, 25))
    return f


def step_run(P, L, inputs, theta):
    f = new_filter(P, L, inputs)
    one = stepper(f, inputs, theta)
    for s in range(WARM):
        one(s)
    f.synchronize()
    t0 = time.perf_counter()
    for s in range(WARM, WARM + STEPS):
        one(s)
    f.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / STEPS
    poses = f.download_poses()[:, :3]
    f.close()
    return ms, poses


def what_it_buys(emit, P=10000, L=500, steps=64):
    inputs = inputs_for(L, steps)
    for theta in (None, 0.5, 0.25):
        f = new_filter(P, L, inputs)
        f.path_enable(RING)
        one = stepper(f, inputs, theta)
        n_eff = []
        for s in range(steps):
            one(s)
            if theta is not None and s % 8 == 7:
                n_eff.append(round(f.resample_stats().n_eff / P, 4))
        surv = f.path_summary().survivors
        emit(dict(what="what it buys", particles=P, landmarks=L, steps=steps, ring=RING, threshold=theta,
                  resamples=steps if theta is None else f.resample_stats().resamples,
                  survivors_at_rows_0_16_32_48=[int(surv[t]) for t in (0, 16, 32, 48)], survivors_current=int(surv[-1]),
                  n_eff_over_P_every_8th_step=n_eff))
        f.close()


def summary_cost(emit, P):
    rs = np.random.RandomState(3)
    f = _lib.DeviceFilter(P, 0)
    poses = np.column_stack([rs.uniform(-1.0, 1.0, (P, 3)), rs.uniform(0.1, 1.0, P) ** 4])
    f.upload_poses(poses)
    out = {}
    for name, call in (("pk_summary", f.summary), ("pk_summary_weighted", lambda: f.summary_weighted(LOG))):
        call()  # (buffers, first touch)
        f.enable_timing(SUMMARY_BIT)
        f.reset_timings()
        t0 = time.perf_counter()
        for _ in range(20):
            call()
        wall = (time.perf_counter() - t0) * 1e3 / 20
        ms, n = f.timings()["summary"]
        f.enable_timing(False)
        out[name] = dict(device_ms_per_call=round(ms / 20, 5), bracketed_spans=n, host_wall_ms_per_call=round(wall, 4))
    emit(dict(what="summary call", particles=P, calls=20, **out))
    f.close()


def four_steps(mode, P=10000, L=500):
    inputs = inputs_for(L, 4)
    f = new_filter(P, L, inputs)
    one = stepper(f, inputs, None if mode == "plain" else 0.5)
    for s in range(4):
        one(s)
    f.synchronize()
    print(json.dumps(dict(what="four steps", mode=mode, particles=P, landmarks=L, summary=f.summary())), flush=True)
    f.close()


if __name__ == "__main__":
    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.join(ROOT, "parakeet_slam_amd", sys.argv[sys.argv.index("--lib") + 1])
        import ctypes

        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in ADAPTIVE_SYMBOLS:  # a build from before these entry points: bind what it has
            if not hasattr(probe, name):
                _lib.SIGNATURES.pop(name, None)
    if "--four-steps" in sys.argv:
        four_steps(sys.argv[sys.argv.index("--four-steps") + 1])
        sys.exit(0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "adaptive_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)
        return ln

    P, L = arg("--particles", bench.DEFAULT_P), arg("--landmarks", bench.DEFAULT_L)
    inputs = inputs_for(L, WARM + STEPS)
    step_run(min(P, 4096), L, inputs, 2.0)  # (the process's first launches, code objects loaded: not a figure)
    plain, gated, same = [], [], True
    for run in range(RUNS):
        poses = {}
        for theta in (None, 2.0):
            ms, poses[theta] = step_run(P, L, inputs, theta)
            (plain if theta is None else gated).append(ms)
            emit(dict(what="step", particles=P, landmarks=L, entry="pk_step" if theta is None else "pk_step_adaptive(threshold 2)", run=run,
                      ms_per_step=round(ms, 4)))
        same = same and np.array_equal(poses[None], poses[2.0])
    spread = (max(plain) - min(plain)) / np.median(plain)
    ratio = float(np.median(gated) / np.median(plain))
    emit(dict(what="pk_step against pk_step_adaptive(threshold 2)", particles=P, landmarks=L, steps=STEPS, runs=RUNS,
              pk_step_ms=[round(v, 4) for v in plain], adaptive_ms=[round(v, 4) for v in gated],
              pk_step_median=round(float(np.median(plain)), 4), adaptive_median=round(float(np.median(gated)), 4),
              pk_step_range=[round(min(plain), 4), round(max(plain), 4)], adaptive_range=[round(min(gated), 4), round(max(gated), 4)],
              adaptive_over_pk_step=round(ratio, 5), pk_step_spread_max_minus_min_over_median=round(float(spread), 5),
              difference_resolved_by_the_spread=bool(abs(ratio - 1.0) > spread), same_poses_after_every_run=bool(same)))
    what_it_buys(emit)
    summary_cost(emit, P)
    fh.close()

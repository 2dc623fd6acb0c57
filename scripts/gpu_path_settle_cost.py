"""What the trunk of the path estimate costs (pk_path_trunk_enable, pk_path_settle; pk_k_path_settle.hip) on one GPU.  After
gpu_path_weighted_cost.py's and gpu_path_cost.py's method; one call, one JSON line per figure, into --out (default
out/path_settle_cost.json) and beside it the two kernel-stats tables:
  1. before this process opens the GPU: `rocprofv3 --kernel-trace --stats` (no counters) over four plain steps of a 10 000 x 500
     filter in a child process, once with the package's library and once with --parent-lib (a build of the parent commit, placed
     beside the package's; skipped when it is not there): with recording off the kernels and their counts must be the same;
  2. one settle at 100 000 particles: E = 16 of 64 rows and E = 256 of 1 024, on a ring that coalesces (pk_resample of uneven
     weights at every row) and on one where every lineage survives (pk_resample_adaptive with threshold 0: identity ancestors).
     pk_path_summary_weighted -- unchanged, so the parent's figure -- against pk_path_settle on the same ring in the same process,
     alternating: per round one weighted summary, one settle, then E records that fill the ring again.  One untimed round, 20
     timed; PK_T_SUMMARY hipEvents per call, the median and the spread (max - min over the median) of each;
  3. the headline step (bench.py's workload, 100 000 x 2 000 through pk_step) three ways, five fresh filters each, alternating:
     recording on without a trunk, with a ring of 64 settled 16 rows at a time, with a ring of 1 024 settled 256 at a time.  Every
     way of a pair runs the same steps: the ring is filled first, the timed steps span whole batches.
--four-steps: nothing but the four steps (what the children run); --lib NAME: another build of the library beside the package's.
    python scripts/gpu_path_settle_cost.py [--out FILE] [--particles P] [--landmarks L] [--parent-lib NAME] [--skip-steps]"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from parakeet_slam_amd import _lib  # noqa: E402

CALLS, RUNS = 20, 5
SUMMARY_BIT = 1 << _lib.PK_T_NAMES.index("summary")
LOG = _lib.PK_WEIGHTS_LOG
NEW_SYMBOLS = ("pk_path_trunk_enable", "pk_path_settle", "pk_path_trunk_shape", "pk_path_trunk_download", "pk_path_trunk_upload",
               "pk_path_trunk_summary")


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def four_steps(P=10000, L=500):
    import random

    import bench

    means, covs, scans = bench.synthetic_inputs(L, 4)
    ws = bench.synthetic_controls(4)
    rnd = random.Random(7)
    f = _lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    for s in range(4):
        f.step(0.2, ws[s], 0.1, scans[s], rnd.random(), seed=7, draw=s, domain=LOG)
    f.synchronize()
    print(json.dumps(dict(what="four steps", particles=P, landmarks=L, summary=f.summary())), flush=True)
    f.close()


def kernel_counts(out_dir, name, lib):
    """One child under rocprofv3: {kernel: calls} from its stats table, which is copied beside the figures."""
    work = os.path.join(out_dir, "trace_" + name)
    shutil.rmtree(work, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable, os.path.abspath(__file__),
           "--four-steps"] + (["--lib", lib] if lib else [])
    subprocess.run(cmd, check=True, timeout=280, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    tables = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
    assert len(tables) == 1, tables
    kept = os.path.join(out_dir, "kernel_stats_four_steps_%s.csv" % name)
    shutil.copyfile(tables[0], kept)
    shutil.rmtree(work, ignore_errors=True)
    with open(kept) as fh:
        return {row["Name"]: int(row["Calls"]) for row in csv.DictReader(fh)}


def uneven(rs, P):
    logw = rs.uniform(-30.0, 0.0, P)
    logw[rs.permutation(P)[:P // 10]] = -np.inf
    return logw


def record_rows(f, n, kind, rs, draw0):
    for s in range(n):
        f.motion(0.3, 0.1, 0.1, seed=11, draw=draw0 + s)
        if kind == "coalescing":
            if (draw0 + s) % 16 == 0:  # (fresh uneven weights now and then; in between pk_resample carries the chosen particles' along)
                f.upload_log_weights(rs.uniform(-3.0, 0.0, f.P))
            f.resample(float(rs.uniform(0.0, 1.0)), domain=LOG)
        else:
            f.resample_adaptive(float(rs.uniform(0.0, 1.0)), 0.0, domain=LOG)


def one_call_ms(f, call):
    f.reset_timings()
    call()
    f.synchronize()
    return f.timings()["summary"][0]


def figures(ms):
    ms = np.asarray(ms)
    return dict(device_ms_median=round(float(np.median(ms)), 5), device_ms_min=round(float(ms.min()), 5), device_ms_max=round(float(ms.max()), 5),
                spread_max_minus_min_over_median=round(float((ms.max() - ms.min()) / np.median(ms)), 5))


def settle_cost(emit, P, rows, E, kind):
    """A ring of rows + 1 that holds `rows` whenever it is measured: the automatic settle, which needs a full ring, never runs."""
    rs = np.random.RandomState(rows + len(kind))
    f = _lib.DeviceFilter(P, 0)
    f.upload_poses(np.column_stack([rs.uniform(10.0, 20.0, P), rs.uniform(-5.0, 5.0, P), rs.uniform(-0.6, 0.6, P), np.ones(P)]))
    f.path_enable(rows + 1)
    f.path_trunk_enable(rows + 1)
    record_rows(f, rows, kind, rs, 0)
    draw = rows
    weighted, settle, survivors = [], [], None
    f.enable_timing(SUMMARY_BIT)
    for call in range(CALLS + 1):
        f.upload_log_weights(uneven(rs, P))
        assert f.path_shape()[1] == rows
        if call == 1:
            survivors = f.path_summary().survivors
        w = one_call_ms(f, lambda: f.path_summary_weighted(LOG))
        f.synchronize()
        s = one_call_ms(f, lambda: f.path_settle(E, LOG))
        if call:  # (the first round: buffers, first touch)
            weighted.append(w)
            settle.append(s)
        record_rows(f, E, kind, rs, draw)
        draw += E
    f.enable_timing(False)
    _, first, length = f.path_trunk_shape()
    final = int(np.sum(np.ptp(f.path_trunk_summary(first + length - E, first + length)[2], axis=1) == 0))
    out = dict(pk_path_summary_weighted=figures(weighted), pk_path_settle=figures(settle))
    ratio = out["pk_path_settle"]["device_ms_median"] / out["pk_path_summary_weighted"]["device_ms_median"]
    emit(dict(what="one settle against pk_path_summary_weighted", particles=P, rows_held=rows, rows_settled=E, ring=kind, calls=CALLS,
              survivors_row_0=int(survivors[0]), survivors_row_E=int(survivors[E]), final_rows_of_the_last_settle=final,
              settle_over_weighted=round(ratio, 4), settle_ms_per_settled_row=round(out["pk_path_settle"]["device_ms_median"] / E, 6),
              faster_by_more_than_the_weighted_calls_spread=bool(
                  1.0 - ratio > out["pk_path_summary_weighted"]["spread_max_minus_min_over_median"]), **out))
    f.close()


def step_run(P, L, inputs, ring, batch, warm, steps):
    means, covs, scans, ws, us = inputs
    n = len(scans)
    f = _lib.DeviceFilter(P, L)
    f.upload_map(means, covs.reshape(L, 25))
    f.path_enable(ring)
    if batch:
        f.path_trunk_enable(batch)

    def one(s):
        f.step(0.2, ws[s % n], 0.1, scans[s % n], us[s % n], seed=7, draw=s, domain=LOG)

    for s in range(warm):
        one(s)
    f.synchronize()
    t0 = time.perf_counter()
    for s in range(warm, warm + steps):
        one(s)
    f.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    shape = f.path_shape() + (f.path_trunk_shape() if batch else ())
    summary = f.summary()
    f.close()
    return ms, shape, summary


def step_cost(emit, P, L):
    import random

    import bench

    n = 64
    means, covs, scans = bench.synthetic_inputs(L, n)
    rnd = random.Random(7)
    inputs = (means, covs, scans, bench.synthetic_controls(n), [rnd.random() for _ in range(n)])
    step_run(min(P, 4096), L, inputs, 8, 2, 8, 8)  # (the process's first launches, code objects loaded: not a figure)
    for ring, batch in ((64, 16), (1024, 256)):
        warm, steps = ring, 4 * batch if ring == 64 else batch  # the ring fills in the warm-up; the timed steps span whole batches
        off, on, summaries = [], [], set()
        for run in range(RUNS):
            for b in (0, batch):
                ms, shape, summary = step_run(P, L, inputs, ring, b, warm, steps)
                (on if b else off).append(ms)
                summaries.add(summary)
                emit(dict(what="step", particles=P, landmarks=L, ring=ring, batch=b, run=run, ms_per_step=round(ms, 4), shapes=shape))
        spread = (max(off) - min(off)) / np.median(off)
        extra = float(np.median(on) - np.median(off))
        emit(dict(what="recording without a trunk against with", particles=P, landmarks=L, ring=ring, batch=batch, warm_steps=warm,
                  timed_steps=steps, runs=RUNS, without_ms=[round(v, 4) for v in off], with_ms=[round(v, 4) for v in on],
                  without_median=round(float(np.median(off)), 4), with_median=round(float(np.median(on)), 4),
                  with_over_without=round(float(np.median(on) / np.median(off)), 5),
                  without_spread_max_minus_min_over_median=round(float(spread), 5), extra_ms_per_step=round(extra, 5),
                  same_summary_in_every_run=len(summaries) == 1))


if __name__ == "__main__":
    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.join(ROOT, "parakeet_slam_amd", sys.argv[sys.argv.index("--lib") + 1])
        import ctypes

        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_SYMBOLS:  # a build from before these entry points: bind what it has
            if not hasattr(probe, name):
                _lib.SIGNATURES.pop(name, None)
    if "--four-steps" in sys.argv:
        four_steps()
        sys.exit(0)
    out_path = arg("--out", os.path.join("out", "path_settle_cost.json"), str)
    out_dir = os.path.dirname(os.path.abspath(out_path))
    os.makedirs(out_dir, exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)

    parent = arg("--parent-lib", "libpk_parent.so", str)
    tree = kernel_counts(out_dir, "tree", None)
    if os.path.exists(os.path.join(ROOT, "parakeet_slam_amd", parent)):
        old = kernel_counts(out_dir, "parent", parent)
        emit(dict(what="four plain steps, kernels and their counts", particles=10000, landmarks=500, kernels=len(tree),
                  launches=sum(tree.values()), same_as_parent=bool(tree == old),
                  differences={k: [old.get(k), tree.get(k)] for k in sorted(set(old) | set(tree)) if old.get(k) != tree.get(k)}))
    else:
        emit(dict(what="four plain steps, kernels and their counts", kernels=len(tree), launches=sum(tree.values()), same_as_parent=None,
                  note="%s is not beside the package's library: nothing to compare with" % parent))
    P = arg("--particles", 100000)
    for rows, E in ((64, 16), (1024, 256)):
        for kind in ("coalescing", "every lineage survives"):
            settle_cost(emit, P, rows, E, kind)
    if "--skip-steps" not in sys.argv:
        import bench

        step_cost(emit, P, arg("--landmarks", bench.DEFAULT_L))
    fh.close()

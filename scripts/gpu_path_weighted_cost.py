"""What the weighted path estimate costs (pk_path_summary_weighted; pk_k_path_weighted.hip) against pk_path_summary on one GPU.
After gpu_path_cost.py's and gpu_adaptive_cost.py's method; one call, one JSON line per figure, into --out (default
out/path_weighted_cost.json) and beside it the two kernel-stats tables:
  1. before this process opens the GPU: `rocprofv3 --kernel-trace --stats` (no counters) over four plain steps of a 10 000 x 500
     filter in a child process, once with the package's library and once with --parent-lib (a build of the parent commit, placed
     beside the package's; skipped when it is not there): the kernels and their counts must be the same;
  2. 100 000 particles with 64 and 1 024 rows held, on a ring that coalesces (pk_resample of uneven weights at every row) and on one
     where every lineage survives (pk_resample_adaptive with threshold 0: identity ancestors), and at 64 rows on one of random
     permutations (path_upload: every lineage survives and every gather is scattered): pk_path_summary -- unchanged, so the parent's
     figure -- against pk_path_summary_weighted on the same ring in the same
     process, 20 calls each behind one untimed call, PK_T_SUMMARY hipEvents and host wall clock.
--four-steps: nothing but the four steps (what the children run); --lib NAME: another build of the library beside the package's.
    python scripts/gpu_path_weighted_cost.py [--out FILE] [--particles P] [--parent-lib NAME]"""
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

CALLS = 20
SUMMARY_BIT = 1 << _lib.PK_T_NAMES.index("summary")
LOG = _lib.PK_WEIGHTS_LOG
NEW_SYMBOLS = ("pk_path_summary_weighted", "pk_best_particle")


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


def build_ring(P, rows, kind, rs):
    f = _lib.DeviceFilter(P, 0)
    f.upload_poses(np.column_stack([rs.uniform(10.0, 20.0, P), rs.uniform(-5.0, 5.0, P), rs.uniform(-0.6, 0.6, P), np.ones(P)]))
    f.path_enable(rows)
    if kind == "permutations":
        poses = np.stack([np.column_stack([rs.uniform(10.0, 20.0, P), rs.uniform(-5.0, 5.0, P), rs.uniform(-0.6, 0.6, P)]) for _ in range(rows)])
        f.path_upload(poses, np.stack([rs.permutation(P) for _ in range(rows)]).astype(np.int32))
    else:
        for s in range(rows):
            f.motion(0.3, 0.1, 0.1, seed=11, draw=s)
            if kind == "coalescing":
                if s % 16 == 0:  # (fresh uneven weights now and then; in between pk_resample carries the chosen particles' along)
                    f.upload_log_weights(rs.uniform(-3.0, 0.0, P))
                f.resample(float(rs.uniform(0.0, 1.0)), domain=LOG)
            else:
                f.resample_adaptive(float(rs.uniform(0.0, 1.0)), 0.0, domain=LOG)
    f.upload_log_weights(uneven(rs, P))
    assert f.path_shape()[1] == rows
    return f


def timed(f, call):
    call()  # (buffers, first touch)
    f.synchronize()
    f.enable_timing(SUMMARY_BIT)
    f.reset_timings()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        call()
    wall = (time.perf_counter() - t0) * 1e3 / CALLS
    ms, n = f.timings()["summary"]
    f.enable_timing(False)
    return dict(device_ms_per_call=round(ms / CALLS, 5), bracketed_spans=int(n), host_wall_ms_per_call=round(wall, 4))


def ring_cost(emit, P, rows, kind):
    rs = np.random.RandomState(rows + len(kind))
    f = build_ring(P, rows, kind, rs)
    surv = f.path_summary().survivors
    out = dict(pk_path_summary=timed(f, f.path_summary))
    out["pk_path_summary_weighted"] = timed(f, lambda: f.path_summary_weighted(LOG))
    base = out["pk_path_summary"]["device_ms_per_call"]
    emit(dict(what="path summary call", particles=P, rows_held=rows, ring=kind, calls=CALLS, survivors_row_0=int(surv[0]),
              survivors_middle_row=int(surv[rows // 2]), launches_pk_path_summary=rows + 3, launches_weighted=5,
              weighted_over_pk_path_summary=round(out["pk_path_summary_weighted"]["device_ms_per_call"] / base, 4), **out))
    f.close()


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
    out_path = arg("--out", os.path.join("out", "path_weighted_cost.json"), str)
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
    for rows, kind in ((64, "coalescing"), (64, "every lineage survives"), (64, "permutations"), (1024, "coalescing"),
                       (1024, "every lineage survives")):
        ring_cost(emit, P, rows, kind)
    fh.close()

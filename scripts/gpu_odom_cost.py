"""What the odometry motion model costs, and that the twist-driven step costs what it did (k_motion_odom, pk_k_motion_odom.hip;
DESIGN.md section 4, "The odometry motion model") on one GPU.  After gpu_path_settle_cost.py's method; one JSON line per figure:
  1. the kernel: `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) over a child that launches k_motion and
     k_motion_odom alternately, 50 times each, at 100 000 particles with device noise: calls, mean and minimum of both.  k_motion is
     unchanged, so its figure is the parent's; the two move the same bytes and draw the same normals.  No bar beyond "no scratch".
  2. the twist path: the same trace over four plain pk_step of a 10 000 x 500 filter, once with the package's library and once with
     --parent-lib (a build of the parent commit, placed beside it): the same kernels with the same counts.
  3. --parent-checkout DIR (a checkout of the parent commit with its own built library): `bench.py --gpus 1 --steps 20 --warmup 5`
     (headline only) there and in this tree, alternating, two runs each; all four figures.
Every GPU process is a child with a time limit; the first that fails ends the script.
    python scripts/gpu_odom_cost.py [--out FILE] [--parent-lib NAME] [--parent-checkout DIR]"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from parakeet_slam_amd import _lib  # noqa: E402

LOG = _lib.PK_WEIGHTS_LOG
NEW_SYMBOLS = ("pk_odom_delta", "pk_odom_sigmas", "pk_motion_odom", "pk_motion_odom_range", "pk_step_odom")
ALPHAS = (0.0025, 0.0001, 0.0025, 0.0001)
BENCH = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-secondary", "--no-probes", "--no-configs4", "--no-refscene"]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def alternate(P=100000, calls=50):
    f = _lib.DeviceFilter(P, 0)
    delta = _lib.odom_delta((0.0, 0.0, 0.0), (0.02, 0.002, 0.01))  # 0.2 m/s, 0.1 rad/s over 0.1 s: the twist's own step
    for s in range(calls):
        f.motion(0.2, 0.1, 0.1, seed=7, draw=2 * s)
        f.motion_odom(delta, ALPHAS, seed=7, draw=2 * s + 1)
    f.synchronize()
    print(json.dumps(dict(what="alternate", particles=P, calls=calls, summary=f.summary())), flush=True)
    f.close()


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


def kernel_stats(out_dir, name, mode, lib=None):
    """One child under rocprofv3: its kernel stats table (copied beside the figures) as {kernel: row}."""
    work = os.path.join(out_dir, "trace_" + name)
    shutil.rmtree(work, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable, os.path.abspath(__file__),
           mode] + (["--lib", lib] if lib else [])
    subprocess.run(cmd, check=True, timeout=280, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    tables = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
    assert len(tables) == 1, tables
    kept = os.path.join(out_dir, "kernel_stats_%s.csv" % name)
    shutil.copyfile(tables[0], kept)
    shutil.rmtree(work, ignore_errors=True)
    with open(kept) as fh:
        return {row["Name"]: row for row in csv.DictReader(fh)}


def bench_line(where):
    out = subprocess.run([sys.executable, "bench.py"] + BENCH, cwd=where, check=True, timeout=560, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL).stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("{") and '"metric"' in ln]
    return json.loads(lines[-1])


if __name__ == "__main__":
    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.join(ROOT, "parakeet_slam_amd", arg("--lib", None))
        import ctypes

        probe = ctypes.CDLL(_lib.LIB_PATH)
        for sym in NEW_SYMBOLS:  # a build from before these entry points: bind what it has
            if not hasattr(probe, sym):
                _lib.SIGNATURES.pop(sym, None)
    if "--alternate" in sys.argv:
        alternate()
        sys.exit(0)
    if "--four-steps" in sys.argv:
        four_steps()
        sys.exit(0)
    out_path = arg("--out", os.path.join("out", "odom_cost.json"))
    out_dir = os.path.dirname(out_path) or "."
    os.makedirs(out_dir, exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)

    rows = kernel_stats(out_dir, "motion_alternating", "--alternate")
    fig = {}
    for kernel, row in rows.items():
        for key in ("k_motion_odom", "k_motion"):
            if kernel.startswith("pk::%s(" % key):
                fig[key] = dict(calls=int(row["Calls"]), mean_ns=round(float(row["AverageNs"]), 1), min_ns=int(row["MinNs"]),
                                max_ns=int(row["MaxNs"]))
    emit(dict(what="k_motion against k_motion_odom, alternating", particles=100000, **fig,
              odom_over_twist_mean=round(fig["k_motion_odom"]["mean_ns"] / fig["k_motion"]["mean_ns"], 4)))
    tree = {k: int(r["Calls"]) for k, r in kernel_stats(out_dir, "four_steps_tree", "--four-steps").items()}
    parent = arg("--parent-lib", "libpk_parent.so")
    if os.path.exists(os.path.join(ROOT, "parakeet_slam_amd", parent)):
        old = {k: int(r["Calls"]) for k, r in kernel_stats(out_dir, "four_steps_parent", "--four-steps", parent).items()}
        emit(dict(what="four plain steps, kernels and their counts", kernels=len(tree), launches=sum(tree.values()),
                  same_as_parent=bool(tree == old), only_here=sorted(set(tree) - set(old)), only_parent=sorted(set(old) - set(tree))))
    else:
        emit(dict(what="four plain steps, kernels and their counts", kernels=len(tree), launches=sum(tree.values()), same_as_parent=None,
                  note="%s is not beside the package's library: nothing to compare with" % parent))
    checkout = arg("--parent-checkout", None)
    if checkout:
        for repeat in (1, 2):
            for build, where in (("parent", checkout), ("tree", ROOT)):
                ln = bench_line(where)
                emit(dict(what="bench.py", build=build, repeat=repeat, ms_per_step=ln.get("ms_per_step"), summary=ln.get("summary")))
    fh.close()

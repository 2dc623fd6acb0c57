#!/usr/bin/env python3
"""Headline benchmark: FastSLAM filter steps on synthetic 360-degree bearing+colour scans.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--particles P] [--landmarks L]
                    [--assoc ml|known] [--dump-outputs DIR] [--full [--no-cpu-baseline] [--no-secondary] ...]

One "step" = one whole cam_cb (prkt_core_v2.py:59-137): weight reset, motion sample,
maximum-likelihood data association, per particle x landmark EKF update + weight,
systematic resample -- all on the GPU through the C ABI (include/parakeet_slam.h).
The default workload is BASELINE.json configs[2], the largest single-GPU configuration:
100 000 particles x 2 000 landmarks per GPU, B = L blobs per scan, float64 like the
reference; configs[1] (10 000 x 500) rides along as a secondary object at N = 1.

N > 1: one process per GPU, particles sharded, weak scaling.  Started as the driver does
(`python -m torch.distributed.run ... bench.py --gpus N`) the ranks find RANK / WORLD_SIZE in
the environment; started bare (`python bench.py --gpus N`) the script launches those N ranks
itself as child processes BEFORE it touches the GPU and relays rank 0's line.  `n_gpus` is
the world size RCCL actually formed, and it must equal --gpus.

Prints ONE JSON line on rank 0 (contract in the task description).  A plain run sets up,
warms up, times the K steps and reports them, with "roofline" for the dominant kernel of the
timed route (timed with hipEvents on the library's own stream inside the timed region).
Everything that takes work of its own moves behind --full: the untimed probes behind the
timed region, configs[1] and the configs[4] shard, the facade at the reference's scene
sizes, the measured copy bandwidth and "cpu_baseline" (the NumPy oracle of the same step on
a bounded sample of the same workload); the --no-* options switch parts of it off.

--dump-outputs DIR writes what the timed path computed in its last step, before anything
else touches the filter: poses.npy (P x 4: x, y, heading, weight; a seeded sample of rows,
pose_particles.npy, when P is in the millions), summary.npy, and the landmarks of a fixed,
seeded sample of particles (sample_particles.npy, landmark_means.npy, landmark_covs.npy,
landmark_counts.npy), all float64 and at most 64 MB together.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import random
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {  # BASELINE.json configs by (particles per GPU, landmarks)
    (10000, 500): "configs[1]",
    (100000, 2000): "configs[2]",
    (125000, 5000): "configs[4] (one of its eight shards)",
}
DEFAULT_P, DEFAULT_L = 100000, 2000  # configs[2]: the largest single-GPU configuration
SECOND_P, SECOND_L = 10000, 500      # configs[1]


_CODE_NOW = None


def code_now():
    """{kernel: hash of its instructions in the library this run loads} (parakeet_slam_amd/codeobj.py) -- what every replayed counter
    value below is held against: a profiles/*/pmc_*.json file says which instructions it measured (`code`), and a value measured on
    OTHER instructions is not replayed."""
    global _CODE_NOW
    if _CODE_NOW is None:
        try:
            from parakeet_slam_amd import _lib, codeobj

            so = os.path.join(ROOT, "parakeet_slam_amd", os.environ["PK_BENCH_LIB"]) if os.environ.get("PK_BENCH_LIB") else _lib.LIB_PATH
            _CODE_NOW = codeobj.figures(so)
        except Exception as e:  # noqa: BLE001
            _CODE_NOW = {"error": repr(e)}
    return _CODE_NOW


TRAFFIC_KERNEL = {"step_pub": "k_step_pub<2, 512>", "step_pub_big": "k_step_pub_big", "step_pub_duo": "k_step_pub_duo", "step_fused": "k_step_fused",
                  "step_regs": "k_step_regs", "observe_known": "k_observe"}


def same_code(doc, kernel_key):
    """Did the counter file `doc` measure the instructions this run executes for `kernel_key`?  (True / False, reason)"""
    now, then = code_now().get(kernel_key), (doc.get("code") or {}).get(kernel_key)
    if now is None:
        return False, "this run cannot hash the loaded library's %s (%s)" % (kernel_key, code_now().get("error", "no such kernel"))
    if then is None:
        return False, "the file does not say which instructions it measured (made before round 6)"
    if now != then:
        return False, "measured on other instructions of %s (file %s, this library %s)" % (kernel_key, then, now)
    return True, "same instructions of %s (%s)" % (kernel_key, now)


def measured_traffic(P, L, variant, notes=None, kernel_key=None):
    """HBM bytes per launch of the route's dominant kernel from the committed rocprofv3 PMC run
    (profiles/*/pmc_traffic*.json, made by scripts/gpu_pmc_traffic.sh) when it was taken on this very
    configuration AND on the instructions this run's library holds, else None.  The newest round wins."""
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for rnd in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        rdir = os.path.join(pdir, rnd)
        if not os.path.isdir(rdir):
            continue
        for name in sorted(os.listdir(rdir)):
            if not (name.startswith("pmc_traffic") and name.endswith(".json")):
                continue
            try:
                d = json.load(open(os.path.join(rdir, name)))
            except ValueError:
                continue
            if d["config"]["particles"] == P and d["config"]["landmarks"] == L and variant in d["bytes_per_launch"]:
                ok, why = same_code(d, kernel_key or TRAFFIC_KERNEL.get(variant, variant))  # (kernel_key: "step_pub" is k_step_pub<1, 256> up to 512 landmarks)
                best = d["bytes_per_launch"][variant] if ok else None
                if notes is not None:
                    notes["traffic"] = "profiles/%s/%s (git %s): %s" % (rnd, name, d.get("git", "?"), why)
    return best


def measured_traffic_window(P, L, route, notes=None):
    """The same counters over the DRIVER'S WINDOW (scripts/gpu_pmc_window.sh: the mean over the 25 launches of bench.py --steps 20
    --warmup 5 at this size, profiles/*/pmc_traffic_window_*.json), or None.  The newest round wins."""
    key = SQ_KERNEL_KEY.get(route)
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for rnd in sorted(os.listdir(pdir)) if (key and os.path.isdir(pdir)) else []:
        rdir = os.path.join(pdir, rnd)
        for name in sorted(os.listdir(rdir)) if os.path.isdir(rdir) else []:
            if not (name.startswith("pmc_traffic_window") and name.endswith(".json")):
                continue
            try:
                d = json.load(open(os.path.join(rdir, name)))
            except ValueError:
                continue
            if d["config"]["particles"] == P and d["config"]["landmarks"] == L:
                for k, v in d["bytes_per_launch"].items():
                    if k.startswith(key):
                        ok, why = same_code(d, key)
                        best = v if ok else None
                        if notes is not None:
                            notes["traffic_window"] = "profiles/%s/%s (git %s): %s" % (rnd, name, d.get("git", "?"), why)
    return best


CLOCK_GHZ = 2.4   # MI355X_MICROARCH.md: peak engine clock
N_SIMD = 1024     # 256 CUs x 4 SIMDs
SQ_KERNEL_KEY = {"ml_regs_pub": "k_step_pub<2, 512>", "ml_fused": "k_step_fused", "ml_fused_pub": "k_step_pub<1, 256>", "ml_pub_big": "k_step_pub_big",
                 "ml_pub_duo": "k_step_pub_duo", "ml_regs": "k_step_regs", "known_ids": "k_observe"}


def measured_issue(P, L, route, notes=None):
    """Instruction-issue time of the route's dominant kernel for one launch over P particles, from the committed SQ counter pass
    (profiles/*/pmc_sq_*.json, scripts/gpu_pmc_sq.sh) taken at THIS map size: VALU wave-instructions per particle x P x 4 cycles /
    (1 024 SIMDs x clock) -- the scalar instructions issue on a port of their own at about a cycle each and are reported beside
    it, not added.  The counts per particle do not depend on P (persistent grid, one particle per workgroup at
    a time).  The newest round wins; None when no pass exists for this size / kernel."""
    import re

    key = SQ_KERNEL_KEY.get(route)
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for rnd in sorted(os.listdir(pdir)) if (key and os.path.isdir(pdir)) else []:
        rdir = os.path.join(pdir, rnd)
        for name in sorted(os.listdir(rdir)) if os.path.isdir(rdir) else []:
            if not (name.startswith("pmc_sq") and name.endswith(".json")):
                continue
            try:
                d = json.load(open(os.path.join(rdir, name)))
                cfg = d["config"]
                mp, ml = re.search(r"--particles (\d+)", cfg), re.search(r"--landmarks (\d+)", cfg)
                if not (mp and ml) or int(ml.group(1)) != L:
                    continue
                for k, c in d["counters"].items():
                    if key in k and c.get("SQ_INSTS_VALU", 0) > 0:
                        ok, why = same_code(d, key)
                        if notes is not None:
                            notes["issue"] = "profiles/%s/%s (git %s): %s" % (rnd, name, d.get("git", "?"), why)
                        if not ok:
                            best = None
                            continue
                        per_particle = c["SQ_INSTS_VALU"] / float(mp.group(1))
                        best = {"ms": per_particle * P * 4.0 / (N_SIMD * CLOCK_GHZ * 1e9) * 1e3,
                                "salu_ms": c.get("SQ_INSTS_SALU", 0.0) / float(mp.group(1)) * P * 1.0 / (N_SIMD * CLOCK_GHZ * 1e9) * 1e3,
                                "valu_per_particle": c["SQ_INSTS_VALU"] / float(mp.group(1)),
                                "salu_per_particle": c.get("SQ_INSTS_SALU", 0.0) / float(mp.group(1)),
                                "source": "profiles/%s/%s (git %s)" % (rnd, name, d.get("git", "?"))}
            except (ValueError, KeyError, OSError):
                continue
    return best


ROUTE_KERNEL = {
    "known_ids": "k_observe<known ids> (fused EKF update + log-weight)",
    "ml_fused": "k_step_fused (association gates + settling of contested blobs + EKF update + log-weight in ONE kernel)",
    "ml_regs": "k_step_regs (L <= 2048: a particle's whole map in registers, two landmarks per lane; association "
               "gates + settling of contested blobs + EKF update + log-weight in ONE pass over the map)",
    "ml_handoff": "k_observe_fast (EKF update + log-weight + settling of contested associations; includes the "
                  "near-empty general k_observe launch for flagged particles; the association kernel is separate)",
    "ml_sweep": "k_observe_sweep (two sweeps over landmark chunks: settling of contested associations, EKF update + "
                "log-weight; the association kernel is separate)",
    "ml_general": "k_observe<ML general> (fused EKF update + log-weight)",
}
ROUTE_KERNEL["ml_regs_pub"] = ("k_step_pub (512 < L <= 2048: a particle's whole map in registers, four landmarks per lane; association gates + "
                               "contested blobs settled by static publish / subscribe through LDS + EKF update + log-weight in ONE pass over the map)")
ROUTE_KERNEL["ml_fused_pub"] = ("k_step_pub<256 lanes> (L <= 512: two landmarks per lane, three workgroups per CU; association gates + contested blobs settled by "
                                "static publish / subscribe through LDS + EKF update + log-weight in ONE pass over the map)")
ROUTE_KERNEL["ml_pub_big"] = ("k_step_pub_big (2048 < L <= 6144: two passes over a particle's map, pair by pair -- gates + verdicts published, contested "
                             "blobs settled through LDS, then rows in again from L2 + EKF update + log-weight + rows out: ONE kernel, no separate association kernel)")
ROUTE_TRAFFIC_KEY = {"known_ids": "observe_known", "ml_fused": "step_fused", "ml_fused_pub": "step_pub", "ml_regs": "step_regs", "ml_regs_pub": "step_pub", "ml_pub_big": "step_pub_big",
                     "ml_handoff": "observe_ml", "ml_sweep": "observe_sweep"}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
BYTES_PER_UPDATE = 224  # 14 fp64 read + 14 written per particle.landmark


def synthetic_controls(steps, w=0.1, dt=0.1):
    """Angular velocity per step.  The reference evaluates |atan2(fy - sy, fx - sx) - blob.bearing|
    > pi/2 with the robot-frame bearing (prkt_core_v2.py:473-475, frames mixed): once the robot's
    heading passes pi/2 EVERY blob gets probability 0 and no EKF update happens any more -- a
    degenerate workload (measured: the step gets 25 % faster).  So SURVEY 8d's control
    (v, w) = (0.2, 0.1) is kept for the first 60 steps of 0.1 s and the robot then turns back
    and forth between -0.6 and +0.6 rad."""
    out, h, sign = [], 0.0, 1.0
    for _ in range(steps):
        if abs(h + sign * w * dt) > 0.6:
            sign = -sign
        out.append(sign * w)
        h += sign * w * dt
    return out


def synthetic_inputs(L, steps, v=0.2, w=0.1, dt=0.1):
    """World + noise-free scans along the true trajectory.  Restated here so the
    timed path does not import the oracle."""
    rs = np.random.RandomState(123)
    phi = -math.pi + 2.0 * math.pi * np.arange(L) / float(L) + 0.01
    rho = rs.uniform(8.0, 30.0, size=L)
    col = rs.uniform(0.0, 255.0, size=(L, 3))
    if os.environ.get("PK_BENCH_LATTICE"):  # experiment: colours on a lattice, no blob passes two landmarks' gates
        n = int(math.ceil(L ** (1.0 / 3.0)))
        idx = np.arange(L)
        col = np.stack([idx % n, (idx // n) % n, idx // (n * n)], axis=1) * (255.0 / max(n - 1, 1))
    means = np.empty((L, 5))
    means[:, 0] = rho * np.cos(phi)
    means[:, 1] = rho * np.sin(phi)
    means[:, 2:] = col
    covs = np.broadcast_to(0.25 * np.identity(5), (L, 5, 5)).copy()
    x = y = h = 0.0
    scans = []
    for ws in synthetic_controls(steps, w, dt):
        h1 = h + ws * dt / 2
        x, y = x + v * dt * math.cos(h1), y + v * dt * math.sin(h1)
        h = math.atan2(math.sin(h1 + ws * dt / 2), math.cos(h1 + ws * dt / 2))
        blobs = np.empty((L, 4))
        blobs[:, 0] = np.arctan2(means[:, 1] - y, means[:, 0] - x) - h
        blobs[:, 1:] = col
        scans.append(blobs)
    return means, covs, scans


def usable_cores():
    """Host cores this process may really use: the affinity mask, capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, n)


def _cpu_run(job):
    """One oracle filter of Ps particles stepped nsteps times; returns its wall time."""
    from oracle.fastslam_oracle import OracleFilter

    try:  # one thread per process, whatever BLAS/OpenMP pools NumPy was built with
        from threadpoolctl import threadpool_limits

        threadpool_limits(1)
    except Exception:
        pass
    L, Ps, nsteps, seed = job
    means, covs, scans = synthetic_inputs(L, nsteps)
    rs = np.random.RandomState(seed)
    rnd = random.Random(seed)
    f = OracleFilter(Ps, means, covs)
    t0 = time.perf_counter()
    for s in range(nsteps):
        f.step(0.2, 0.1, 0.1, rs.standard_normal((Ps, 3)), scans[s], rnd.random())
    return time.perf_counter() - t0


def cpu_baseline(L, budget_s=20.0):
    """NumPy oracle ("port" of the reference step, validated against the reference in tests/)
    timed on a bounded particle sample of the same workload: first on ONE host thread, then on
    every host core with the sample's particles split over a fork()ed process pool (particles
    are independent until the weight sum).  Must run BEFORE the GPU is initialised
    (fork).  `value` is the all-core figure; the 1-thread figure rides along."""
    import multiprocessing as mp

    cores = min(usable_cores(), 64)
    nsteps = 2
    half = budget_s / 2.0
    Ps = 2 if L >= 1500 else 4
    t1 = _cpu_run((L, Ps, nsteps, 7))
    while t1 < half / 1.5 and Ps < 4096:  # the oracle vectorises over particles: grow until the sample fills the budget
        Ps = int(min(4096, max(Ps + 1, Ps * min(8.0, 0.8 * half / t1))))
        t1 = _cpu_run((L, Ps, nsteps, 7))
    single = Ps * L * nsteps / t1
    out = {
        "value": single,
        "unit": "particle*landmark EKF updates/s",
        "cores": 1,
        "kind": "port",
        "steps_per_s": nsteps / t1,
        "single_thread_value": single,
        "sample": "%d particles x %d landmarks x %d blobs, %d full steps (ML association), NumPy oracle, "
        "%.1f s on 1 of %d host cores" % (Ps, L, L, nsteps, t1, os.cpu_count() or 1),
    }
    if cores > 1:
        try:
            with mp.get_context("fork").Pool(cores) as pool:
                # page the workers in; a pool that is much slower than one thread alone (cores
                # fewer than reported) times out and leaves the 1-thread figure
                pool.map_async(_cpu_run, [(L, 2, 1, 7)] * cores).get(timeout=90)
                t0 = time.perf_counter()
                pool.map_async(_cpu_run, [(L, Ps, nsteps, 7 + i) for i in range(cores)],
                               chunksize=1).get(timeout=max(30.0, 6.0 * t1))
                tw = time.perf_counter() - t0
            out.update({
                "value": cores * Ps * L * nsteps / tw,
                "cores": cores,
                "steps_per_s": nsteps / tw,
                "sample": "%d particles (%d per process x %d processes) x %d landmarks x %d blobs, %d full steps "
                "(ML association), NumPy oracle, %.1f s wall on all %d host cores; one thread alone: %.3g updates/s "
                "(%d particles, %.1f s)" % (cores * Ps, Ps, cores, L, L, nsteps, tw, cores, single, Ps, t1),
            })
        except Exception as e:  # a pool that cannot start leaves the 1-thread figure
            out["pool_error"] = repr(e)
    return out


def env_options(filt):
    """Tuning experiments only: PK_OPT_<NAME>=<int> in the environment sets the library option <name> on a filter of this run
    (scripts/gpu_ab_env.sh); the line says so in `env_options`."""
    done = {}
    for name, val in sorted(os.environ.items()):
        if name.startswith("PK_OPT_") and val != "":
            filt.set_option(name[7:].lower(), int(val))
            done[name[7:].lower()] = int(val)
    return done


def workload_name(P, L, assoc):
    tag = CONFIGS.get((P, L))
    head = "BASELINE.json %s" % tag if tag else "custom size (not a BASELINE.json config)"
    return "%s: %d particles/GPU x %d landmarks, B=%d blobs/scan, synthetic 360deg bearing+colour obs, assoc=%s, " \
           "resample every step" % (head, P, L, L, assoc)


def self_launch(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as children (torch.distributed.run,
    one process per GPU) BEFORE anything touches the GPU in this process, relay rank 0's JSON line and
    exit with the launcher's code.  This process never initialises the GPU and never exec()s."""
    import torch

    same_gpu = bool(os.environ.get("PK_BENCH_SAME_GPU"))  # rehearsal on a one-GPU box (gloo): ranks share cuda:0
    ndev = torch.cuda.device_count()  # does not initialise the GPU on this image
    if ndev < args.gpus and not same_gpu:
        sys.stderr.write("bench.py --gpus %d: only %d HIP device(s) visible; not running on fewer GPUs than asked\n"
                         % (args.gpus, ndev))
        raise SystemExit(3)
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this pool
    env["PK_BENCH_CHILD"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    # The ranks run in a process group of their own, so that a launch that does not come back (a rank that never joins, a
    # collective that never completes) can be stopped as a whole, by handle -- no retry, no re-exec: the parent reports and
    # exits non-zero.  The ranks themselves give up on the rendezvous and on any collective after 120 s
    # (init_process_group(timeout=)), which normally ends the launch long before this limit.
    import signal

    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, start_new_session=True)

    def stop_ranks():
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(proc.pid, sig)  # the group we started, nothing else
            except ProcessLookupError:
                break
            try:
                proc.wait(timeout=10)
                break
            except subprocess.TimeoutExpired:
                continue

    # (the ranks' own session no longer hears a SIGTERM / SIGINT sent to this process -- an outer `timeout` would
    # leave them running on the GPU beside whatever starts next.  The parent passes the signal on to the group it started and exits.)
    def on_signal(signum, _frame):
        sys.stderr.write("bench.py --gpus %d: signal %d; stopping the %d ranks\n" % (args.gpus, signum, args.gpus))
        stop_ranks()
        raise SystemExit(128 + signum)

    old = {sig: signal.signal(sig, on_signal) for sig in (signal.SIGTERM, signal.SIGINT)}
    try:
        stdout, _ = proc.communicate(timeout=args.launch_timeout)
    except subprocess.TimeoutExpired:
        sys.stderr.write("bench.py --gpus %d: the %d-rank launch did not finish within %.0f s; stopping it\n"
                         % (args.gpus, args.gpus, args.launch_timeout))
        stop_ranks()
        raise SystemExit(6)
    finally:
        for sig, h in old.items():
            signal.signal(sig, h)
    proc = subprocess.CompletedProcess(cmd, proc.returncode, stdout)
    line = None
    for raw in proc.stdout.decode("utf-8", "replace").splitlines():
        raw = raw.strip()
        if raw.startswith("{") and '"metric"' in raw:
            line = raw
    if proc.returncode != 0 or line is None:
        sys.stderr.write("bench.py --gpus %d: the %d-rank launch failed (exit code %d, %s)\n"
                         % (args.gpus, args.gpus, proc.returncode, "no result line" if line is None else "result line seen"))
        raise SystemExit(proc.returncode or 4)
    rec = json.loads(line)
    # a rehearsal (PK_BENCH_SAME_GPU: every rank on ONE device, gloo) says so and counts DEVICES, not ranks, in n_gpus
    if rec.get("world_size") != args.gpus or (rec.get("n_gpus") != args.gpus and not (same_gpu and rec.get("rehearsal"))):
        sys.stderr.write("bench.py --gpus %d: the ranks report n_gpus = %r, world_size = %r\n"
                         % (args.gpus, rec.get("n_gpus"), rec.get("world_size")))
        raise SystemExit(5)
    sys.stdout.write(line + "\n")
    sys.stdout.flush()
    raise SystemExit(0)


def timed_steps(filt, lib, P, L, K, W, scans, ws, us, ids, barrier, stride):
    """W warm-up steps, then exactly K steps between barriers; hipEvents around the observe launch(es)
    of every stride-th step on the library's stream.  Returns (seconds, timings dict, route)."""
    def one_step(s):
        filt.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, ids=ids, domain=lib.PK_WEIGHTS_LOG)

    # (the warm-up steps one at a time, the stream drained behind each: untimed anyway, and the FIRST scan of a fresh map is the one
    # step of a run that can be out of line -- VERDICT round 5, missing #4 -- so the line says how long each took: timed_steps.warmup_ms)
    timed_steps.warmup_ms, timed_steps.warmup_flagged = [], []
    for s in range(W):
        if hasattr(filt, "synchronize") and hasattr(filt, "observe_flagged") and ids is None:
            filt.synchronize()
            t_w = time.perf_counter()
            one_step(s)
            filt.synchronize()
            timed_steps.warmup_ms.append((time.perf_counter() - t_w) * 1e3)
            timed_steps.warmup_flagged.append(int(filt.observe_flagged()[0]))
        else:
            one_step(s)
    barrier()
    filt.set_option("timing_stride", stride)
    filt.enable_timing(0b0000100)
    filt.reset_timings()
    barrier()
    t0 = time.perf_counter()
    for s in range(W, W + K):
        one_step(s)
    barrier()
    elapsed = time.perf_counter() - t0
    route = filt.observe_route() if hasattr(filt, "observe_route") else ("known_ids" if ids is not None else "ml")
    tm = filt.timings()
    filt.enable_timing(0)
    filt.set_option("timing_stride", 1)
    return elapsed, tm, route, one_step


def per_step_replay(filt, lib, P, L, means, covs, scans, ws, us, ids, first, last, slow=(44, 62)):
    """The same trajectory once more, OUTSIDE the headline's timed region, one step at a time with the stream drained
    around each: wall time per step, particles handed to the fall-back kernels per step.  The timed region itself runs
    asynchronously and cannot be looked into without disturbing it; the replay is bit-identical (same seeds, same draws).
    Returns statistics over the trajectory steps [first, last) -- the timed window -- and over the stretch `slow`, where
    the scene hands the fall-backs the most particles."""
    filt.upload_map(means, covs.reshape(L, 25))
    filt.upload_poses(np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (P, 1)))
    end = min(len(scans), max(last, slow[1] + 1))
    ms, fl, kms = [], [], []
    filt.set_option("timing_stride", 1)
    filt.enable_timing(0b0000100)
    for s in range(end):
        filt.reset_timings()
        filt.synchronize()
        t0 = time.perf_counter()
        filt.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, ids=ids, domain=lib.PK_WEIGHTS_LOG)
        filt.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        fl.append(int(filt.observe_flagged()[0]) if ids is None and hasattr(filt, "observe_flagged") else 0)
        ob = filt.timings()["observe"]
        kms.append(ob[0] / max(ob[1], 1))  # the step's one-pass kernel launch (hipEvents on the library's stream)
    filt.enable_timing(0)

    def stats(a, b):
        a, b = max(a, 0), min(b, end)
        if b <= a:
            return None
        m, f = np.array(ms[a:b]), np.array(fl[a:b])
        return {"trajectory_steps": [a, b - 1], "ms_mean": float(m.mean()), "ms_p95": float(np.percentile(m, 95)), "ms_max": float(m.max()),
                "flagged_particles_mean": float(f.mean()), "flagged_particles_max": int(f.max())}

    worst = int(np.argmax(ms))
    kw = np.array(kms[max(first, 0):min(last, end)])
    return {"what": "untimed replay of the same trajectory, one synchronised step at a time (host wall clock around each step)",
            "timed_window": stats(first, last), "slow_window": stats(slow[0], slow[1] + 1),
            # every step of the run, step 0 -- the first scan of the fresh map -- included (missing #4)
            "all_steps": {"trajectory_steps": [0, end - 1], "ms_max": float(ms[worst]), "argmax_step": worst, "flagged_particles_at_max": int(fl[worst]),
                          "ms_first_steps": [float(v) for v in ms[:6]], "flagged_first_steps": [int(v) for v in fl[:6]],
                          "ms_max_over_timed_window_mean": float(ms[worst] / np.mean(ms[max(first, 0):min(last, end)]))},
            # the one-pass kernel's launch time step by step over the timed window (hipEvents): what frac_range_over_steps is made of
            "kernel_ms_min_max_timed_window": [float(kw.min()), float(kw.max())] if kw.size else None}


DUMP_LIMIT_BYTES = 60 * 10 ** 6  # (under 64 MB, .npy headers included)


def dump_outputs(filt, P, L, out_dir, write=True):
    """What a caller of the timed path receives after its last step, as float64 .npy files under out_dir: the particles' poses
    and weights (all of them, or a seeded sample of rows when they alone would take half the limit: pose_particles.npy), the
    filter's summary, and the landmarks (means, covariances, update counts) of a fixed, seeded sample of particles, as many as
    fit the limit beside the poses.  Called on every rank (the downloads complete a sharded filter's pending exchange); only
    `write` ranks write."""
    poses = np.asarray(filt.download_poses(), dtype=np.float64)
    pose_rows = None
    if poses.nbytes > DUMP_LIMIT_BYTES // 2:
        pose_rows = np.sort(np.random.RandomState(2023).choice(P, DUMP_LIMIT_BYTES // 2 // poses[0].nbytes, replace=False))
        poses = poses[pose_rows]
    summary = np.asarray(filt.summary(), dtype=np.float64)
    per_particle = L * (5 + 25 + 1) * 8
    spent = poses.nbytes + (0 if pose_rows is None else pose_rows.size * 8) + (1 << 20)
    n = int(max(1, min(P, (DUMP_LIMIT_BYTES - spent) // per_particle)))
    sample = np.sort(np.random.RandomState(2024).choice(P, n, replace=False)) if n < P else np.arange(P)
    means = np.empty((n, L, 5))
    covs = np.empty((n, L, 5, 5))
    counts = np.empty((n, L))
    for j, p in enumerate(sample):
        m, c, k = filt.download_landmarks(int(p), int(p) + 1)
        means[j], covs[j], counts[j] = m[0], c[0], k[0]
    if not write:
        return
    os.makedirs(out_dir, exist_ok=True)
    arrays = [("poses", poses), ("summary", summary), ("sample_particles", sample.astype(np.float64)),
              ("landmark_means", means), ("landmark_covs", covs), ("landmark_counts", counts)]
    if pose_rows is not None:
        arrays.append(("pose_particles", pose_rows.astype(np.float64)))
    for name, a in arrays:
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def roofline_object(P, L, route, obs_ms, obs_n, stride, K, copy_gbs):
    obs_avg_s = (obs_ms / max(obs_n, 1)) * 1e-3
    alg_bytes = float(P) * L * BYTES_PER_UPDATE
    achieved = alg_bytes / obs_avg_s / 1e9 if obs_avg_s > 0 else 0.0
    hbm_frac = achieved / HBM_PEAK_GBS
    notes = {}
    issue = measured_issue(P, L, route, notes)
    issue_obj = None
    if issue is not None and obs_avg_s > 0:
        issue_obj = {
            "frac": issue["ms"] / (obs_avg_s * 1e3),
            "issue_ms": issue["ms"],
            "valu_wave_instructions_per_particle": issue["valu_per_particle"],
            "salu_wave_instructions_per_particle": issue["salu_per_particle"],
            "salu_issue_ms": issue.get("salu_ms"),
            "what": "replayed: VALU wave-instructions per launch from the committed SQ counter pass x 4 cycles / (%d SIMDs x "
                    "%.1f GHz) / this run's kernel time -- the share of the launch during which every SIMD would be issuing vector "
                    "instructions if they were spread evenly (a wave64 instruction takes 4 cycles of a SIMD; the scalar instructions "
                    "issue on their own port, about a cycle each: salu_issue_ms, not added)" % (N_SIMD, CLOCK_GHZ),
            "source": issue["source"],
        }
    return {
        "kernel": ROUTE_KERNEL.get(route, route),
        "route": route,
        # the maximum-likelihood kernels are bounded by BOTH the pass over the map and float64 instruction issue: `bound` names the
        # larger share; `frac` / `achieved` stay the HBM figures SURVEY 8(d) defines (ekf_stage is the pure-HBM kernel)
        "bound": "issue" if (issue_obj is not None and issue_obj["frac"] > hbm_frac) else "hbm",
        "issue": issue_obj,
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": measured_traffic(P, L, ROUTE_TRAFFIC_KEY.get(route, "none"), notes, SQ_KERNEL_KEY.get(route)),
        "traffic_source": "builder's rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes on this configuration (separate "
        "passes, bytes = (2*FETCH + WRITE)*1024; FETCH counts Infinity-Cache hits too), replayed from "
        "profiles/*/pmc_traffic*.json -- not collected by this run; null when no pass exists for this size",
        "traffic_window": measured_traffic_window(P, L, route, notes),
        "traffic_window_source": "the same two counters over bench.py --steps 20 --warmup 5 at this size (the driver's window and its warm-up: "
        "mean of the 25 launches), scripts/gpu_pmc_window.sh, replayed from profiles/*/pmc_traffic_window_*.json; `traffic` above is the "
        "pass over three EARLY steps of a fresh filter, where few particles are copies of one ancestor yet; null when no pass exists",
        # which counter files the three replayed figures above came from, and whether they measured the instructions THIS run executes
        # (a file that measured other instructions -- or does not say -- is not replayed: the figure is null)
        "replayed_from": notes,
        "kernel_code": code_now().get(SQ_KERNEL_KEY.get(route, "")),
        "copy_measured": copy_gbs,
        "frac_of_copy": achieved / copy_gbs if copy_gbs else None,
        "avg_launch_ms": obs_avg_s * 1e3,
        "launches": obs_n,
        "launches_note": "hipEvent-bracketed launches inside the timed region (every %d-th step of %d)" % (stride, K),
        "algorithmic_bytes_per_launch": alg_bytes,
        "achieved_note": "algorithmic bytes (224 B per particle.landmark) / launch time: after a resample duplicate "
        "particles read a shared source slot, part of which is served by L2 / Infinity Cache, so this is "
        "NOT all HBM traffic -- see achieved_unique and frac_no_duplicates",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--particles", type=int, default=DEFAULT_P, help="particles per GPU")
    ap.add_argument("--landmarks", type=int, default=DEFAULT_L)
    ap.add_argument("--assoc", choices=["ml", "known"], default="ml")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float64, at most 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: probes, configs[1], the configs[4] shard, the facade objects, the copy "
                         "bandwidth and the CPU baseline (the --no-* options below switch parts of it off)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the configs[1] object")
    ap.add_argument("--no-probes", action="store_true", help="skip the untimed probes behind the timed region")
    ap.add_argument("--no-configs4", action="store_true", help="skip the configs[4] shard object (125 000 x 5 000 on this GPU)")
    ap.add_argument("--no-refscene", action="store_true", help="skip the facade latency object (the reference's own scene sizes)")
    ap.add_argument("--cpu-budget", type=float, default=20.0)
    ap.add_argument("--placement", choices=["balanced", "contiguous"], default=None,
                    help="N > 1: where the resample puts the particles (default: balanced = minimum migration)")
    ap.add_argument("--launch-timeout", type=float, default=float(os.environ.get("PK_BENCH_LAUNCH_TIMEOUT", "1500")),
                    help="N > 1: seconds the parent waits for the ranks before it stops them and exits non-zero")
    ap.add_argument("--force-sharded", action="store_true",
                    help="run the multi-GPU code path (collectives included) even with one rank")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if not args.full:  # a plain run: set-up, warm-up, the timed steps, the outputs, the line -- nothing else
        args.no_cpu_baseline = args.no_secondary = args.no_probes = args.no_configs4 = args.no_refscene = True
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args, sys.argv[1:])  # never returns

    # Exactly ONE line may reach stdout (the JSON).  RCCL and friends print banners to fd 1,
    # so park the real stdout and point fd 1 at stderr until the result is ready.
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: one rank per GPU, no more, no fewer" % (args.gpus, world))
    if os.environ.get("PK_BENCH_SABOTAGE_RANK") in (str(rank), "all"):  # tests: a rank that never joins the process group
        time.sleep(3600)

    import torch

    same_gpu = bool(os.environ.get("PK_BENCH_SAME_GPU"))
    ndev = torch.cuda.device_count()  # does not initialise the GPU
    if ndev == 0:
        raise SystemExit("bench.py needs a GPU: the particle update has no CPU fallback")
    if ndev < world and not same_gpu:
        raise SystemExit("--gpus %d but only %d HIP device(s) visible" % (world, ndev))
    # CPU baseline first: it fork()s a process pool, which must happen before any HIP call.
    # Rank 0 at N=1 only (the other ranks would just wait on it).
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args.landmarks, args.cpu_budget)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the particle update has no CPU fallback")
    if same_gpu:  # rehearsal of the N > 1 control flow on a one-GPU box (with PK_BENCH_BACKEND=gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist

        import datetime

        # every rank says where it runs BEFORE the first collective: a launch that hangs in the rendezvous shows who came
        prop = torch.cuda.get_device_properties(local_rank)
        sys.stderr.write("bench.py rank %d/%d: pid %d, device %d %s uuid %s\n"
                         % (rank, world, os.getpid(), local_rank, prop.name, getattr(prop, "uuid", "?")))
        sys.stderr.flush()
        dist.init_process_group(os.environ.get("PK_BENCH_BACKEND", "gloo" if same_gpu else "nccl"),  # "nccl" = RCCL over xGMI (RCCL refuses two ranks on one device)
                                timeout=datetime.timedelta(seconds=float(os.environ.get("PK_BENCH_DIST_TIMEOUT", "120"))))
        if dist.get_world_size() != args.gpus:
            raise SystemExit("--gpus %d but the process group has %d ranks" % (args.gpus, dist.get_world_size()))
        world = dist.get_world_size()

    from parakeet_slam_amd import _lib

    if os.environ.get("PK_BENCH_LIB"):  # tuning experiments only: A/B of two builds on one box
        _lib.LIB_PATH = os.path.join(ROOT, "parakeet_slam_amd", os.environ["PK_BENCH_LIB"])
    P, L = args.particles, args.landmarks
    K, W = args.steps, args.warmup
    EXTRA = 32  # untimed steps after the timed region (association share, unique sources, supplied-ids route)
    NSC = max(K + W + EXTRA, 64) if args.full else K + W  # (the per-step replay runs through trajectory step 62)
    means, covs, scans = synthetic_inputs(L, NSC)
    ws = synthetic_controls(NSC)
    ids = np.arange(1, L + 1, dtype=np.int32) if args.assoc == "known" else None
    sharded = world > 1 or args.force_sharded

    if sharded:
        import torch.distributed as dist

        if not dist.is_initialized():  # --force-sharded with a single rank
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29577")
            dist.init_process_group("nccl", rank=0, world_size=1)
        from parakeet_slam_amd.sharded import ShardedFilter

        filt = ShardedFilter(P, L, device=local_rank, placement=args.placement)
    else:
        filt = _lib.DeviceFilter(P, L, device=local_rank)
    filt.upload_map(means, covs.reshape(L, 25))
    env_options(filt)
    if os.environ.get("PK_OBSERVE_NV"):  # tuning experiments only
        filt.set_option("observe_landmarks_per_lane", int(os.environ["PK_OBSERVE_NV"]))
    rnd = random.Random(7)
    us = [rnd.random() for _ in range(NSC)]

    def barrier():
        if world > 1:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()
        filt.synchronize()

    # hipEvents around the dominant kernel only (the observe launch), on the library's own stream, inside
    # the timed region.  Two event records cost the stream ~8 us: every launch is bracketed when a step
    # takes milliseconds, every 4th when it takes a fraction of one.
    stride = 1 if float(P) * L >= 5e7 or K < 16 else 4
    if sharded:
        filt.synchronize()
        filt.total_migrated = 0
    elapsed, tm, route, one_step = timed_steps(filt, _lib, P, L, K, W, scans, ws, us, ids, barrier, stride)
    head_warm = {"ms": [round(v, 4) for v in timed_steps.warmup_ms], "flagged_particles": list(timed_steps.warmup_flagged),
                 "what": "the warm-up steps one at a time (host wall clock, the stream drained around each; untimed): the first scan of a "
                         "fresh map is the slowest step of a run"} if timed_steps.warmup_ms else None
    migrated = None
    if sharded:  # particles whose output slot lies on another rank: pose + whole map travel (the all-to-all's volume)
        filt.synchronize()
        t = torch.tensor([float(filt.total_migrated)], dtype=torch.float64, device="cuda:%d" % local_rank)
        if world > 1:
            import torch.distributed as dist

            if dist.get_backend() == "nccl":
                dist.all_reduce(t)
            else:  # gloo rehearsal: host tensor
                t = t.cpu()
                dist.all_reduce(t)
        migrated = float(t.item()) / max(K, 1)
        migrated_bytes = migrated * filt.f.particle_bytes()
        placement = filt.placement
    summary = filt.summary()
    flagged = filt.observe_flagged() if hasattr(filt, "observe_flagged") else None
    if route in ("ml_regs", "ml_fused") and hasattr(filt, "observe_published") and filt.observe_published():
        route += "_pub"  # which instance of the one-pass route worked on the scans is decided on the device
    if args.dump_outputs:  # the filter as the last timed step left it, before any probe touches it
        dump_outputs(filt, P, L, args.dump_outputs, write=rank == 0)
    # validity probe (untimed): share of the blobs of the last timed scan that the particles, as they
    # stand now, still associate with some landmark (the workload degenerates when this collapses)
    matched = None
    if not sharded and hasattr(filt, "associate") and not args.no_probes:
        if float(P) * L <= 2e7:
            matched = float((filt.associate(scans[W + K - 1]) > 0).mean())
        else:  # P x B ids would be gigabytes: a 512-particle filter stepped through the same scans instead
            side = _lib.DeviceFilter(512, L, device=local_rank)
            side.upload_map(means, covs.reshape(L, 25))
            for s in range(W + K):
                side.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, ids=ids, domain=_lib.PK_WEIGHTS_LOG)
            matched = float((side.associate(scans[W + K - 1]) > 0).mean())
            side.close()
    # the association kernel's share and the number of DISTINCT source slots the observe kernel reads
    # (after a resample several particles descend from one ancestor and read the same slot, so part of
    # the 224 B/update stream is served by L2 / Infinity Cache, not HBM), from a few extra untimed steps
    uniq = []
    if args.full:
        filt.enable_timing(0b0000010)
        filt.reset_timings()
        for s in range(W + K, W + K + (0 if args.no_probes else 8)):
            one_step(s)
            if not sharded and hasattr(filt, "download_sources"):
                uniq.append(int(np.unique(filt.download_sources()).size))
        barrier()
        tm["assoc"] = filt.timings()["assoc"]
        filt.enable_timing(0)

    # the streaming figure without duplicates: the same observe launches back to back WITHOUT resamples,
    # every particle reading its own slot (all particles then sit at one pose: the bytes are the same)
    no_dup = None
    if not sharded and not args.no_probes:
        no_dup = {}
        if args.assoc == "ml":
            # ... first on the map AS THE RUN LEFT IT (round 5): every particle's landmarks copied into its own slot (a download
            # materialises the resample's indirection), then the same scan observed six times without a resample -- the steady
            # state of the filter without the cache's help; the two probes below start from a FRESH map instead (the first
            # updates of a landmark: wide colour blocks, every look-alike still a contender)
            s_last = W + K + (0 if args.no_probes else 8) - 1
            filt.download_landmarks(0, 1)
            filt.observe(scans[s_last], fresh=True)
            filt.enable_timing(0b0000100)
            filt.reset_timings()
            for _ in range(6):
                filt.observe(scans[s_last], fresh=True)
            ms, cnt = filt.timings()["observe"]
            filt.enable_timing(0)
            avg = ms / max(cnt, 1) * 1e-3
            no_dup["ml_steady_state_map"] = {"avg_launch_ms": avg * 1e3, "launches": cnt,
                                             "achieved": float(P) * L * BYTES_PER_UPDATE / avg / 1e9 if avg > 0 else 0.0,
                                             "frac": float(P) * L * BYTES_PER_UPDATE / avg / 1e9 / HBM_PEAK_GBS if avg > 0 else 0.0,
                                             "distinct_source_slots": int(np.unique(filt.download_sources()).size)}
        for tag, pids in (("ml", None), ("supplied_ids", np.arange(1, L + 1, dtype=np.int32))):
            if tag == "ml" and args.assoc != "ml":
                continue
            filt.upload_map(means, covs.reshape(L, 25))
            filt.upload_poses(np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (P, 1)))
            filt.observe(scans[0], ids=pids, fresh=True)
            filt.enable_timing(0b0000100)
            filt.reset_timings()
            for _ in range(6):
                filt.observe(scans[0], ids=pids, fresh=True)
            ms, cnt = filt.timings()["observe"]
            filt.enable_timing(0)
            avg = ms / max(cnt, 1) * 1e-3
            no_dup[tag] = {"avg_launch_ms": avg * 1e3, "launches": cnt,
                           "achieved": float(P) * L * BYTES_PER_UPDATE / avg / 1e9 if avg > 0 else 0.0,
                           "frac": float(P) * L * BYTES_PER_UPDATE / avg / 1e9 / HBM_PEAK_GBS if avg > 0 else 0.0}

    # the EKF stage on its own (SURVEY 8d defines the HBM roofline on it): the same filter, reset to
    # the initial map and poses, stepped with SUPPLIED ids -- whole steps, resample included, exactly
    # what `--assoc known` times -- so both routes' rooflines come from one run
    known = None
    if args.assoc == "ml" and not sharded and not args.no_probes:
        kids = np.arange(1, L + 1, dtype=np.int32)
        kn, kw = (20, 3) if K >= 20 else (K, 2)
        filt.upload_map(means, covs.reshape(L, 25))
        filt.upload_poses(np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (P, 1)))
        for s in range(kw):
            filt.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, ids=kids, domain=_lib.PK_WEIGHTS_LOG)
        filt.enable_timing(0b0000100)
        filt.reset_timings()
        barrier()
        k0 = time.perf_counter()
        for s in range(kw, kw + kn):
            filt.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, ids=kids, domain=_lib.PK_WEIGHTS_LOG)
        barrier()
        k1 = time.perf_counter()
        kms, kcnt = filt.timings()["observe"]
        filt.enable_timing(0)
        kavg = (kms / max(kcnt, 1)) * 1e-3
        known = {
            "what": "the filter reset to its initial state, %d whole steps with ids = 1..L (no association)" % kn,
            "ms_per_step": (k1 - k0) / kn * 1e3,
            "value": float(P) * L * kn / (k1 - k0),
            "kernel": ROUTE_KERNEL["known_ids"],
            "avg_launch_ms": kavg * 1e3,
            "launches": kcnt,
            "achieved": float(P) * L * BYTES_PER_UPDATE / kavg / 1e9 if kavg > 0 else 0.0,
            "frac": float(P) * L * BYTES_PER_UPDATE / kavg / 1e9 / HBM_PEAK_GBS if kavg > 0 else 0.0,
            "frac_no_duplicates": no_dup["supplied_ids"]["frac"] if no_dup else None,
            "unit": "GB/s",
            "traffic": measured_traffic(P, L, "observe_known"),
        }
    replay = None
    if not sharded and not args.no_probes:
        replay = per_step_replay(filt, _lib, P, L, means, covs, scans, ws, us, ids, W, W + K)
    filt.close()
    del filt

    # BASELINE.json configs[1] beside the headline (N = 1, default workload only): same code, the
    # L <= 512 route (k_step_fused)
    second = None
    if world == 1 and not args.force_sharded and not args.no_secondary and (P, L) == (DEFAULT_P, DEFAULT_L) \
            and args.assoc == "ml":
        P2, L2, K2, W2 = SECOND_P, SECOND_L, 120, 10
        m2, c2, s2 = synthetic_inputs(L2, K2 + W2)
        f2 = _lib.DeviceFilter(P2, L2, device=local_rank)
        f2.upload_map(m2, c2.reshape(L2, 25))
        e2, tm2, route2, _ = timed_steps(f2, _lib, P2, L2, K2, W2, s2, synthetic_controls(K2 + W2),
                                          [rnd.random() for _ in range(K2 + W2)], None, barrier2(torch, f2), 4)
        if route2 in ("ml_regs", "ml_fused") and f2.observe_published():
            route2 += "_pub"
        second = {
            "workload": workload_name(P2, L2, "ml"),
            "value": float(P2) * L2 * K2 / e2,
            "unit": "updates/s",
            "steps": K2,
            "warmup": W2,
            "ms_per_step": e2 / K2 * 1e3,
            "filter_steps_per_sec": K2 / e2,
            "roofline": roofline_object(P2, L2, route2, tm2["observe"][0], tm2["observe"][1], 4, K2, None),
        }
        f2.close()
        del f2
        # ... and the same steps through the OTHER one-pass kernel for maps of at most 512 landmarks.  The default at this size is the
        # publish / subscribe instance on candidate lists (three 256-lane workgroups per CU) since the end of round 6 -- "pub_small" = -1 takes
        # it from 5e6 particle.landmarks on, where the whole step is measured no slower (profiles/r06/pub_small_sweep*.log: +3 % at 8 000 x 500,
        # a tie here at configs[1]'s 10 000 x 500, -5 % at 16 000 x 500, -15 % at 100 000 x 256): its kernel is 11 % faster, its per-scan
        # kernels (k_candidates, k_cand_entries, a flag launch: 27 us whatever the number of particles) cost what that gains at this size.
        # Beside it: k_step_fused ("pub_small" = 0), the default of rounds 1-5
        try:
            f3 = _lib.DeviceFilter(P2, L2, device=local_rank)
            f3.set_option("pub_small", 0)
            f3.upload_map(m2, c2.reshape(L2, 25))
            rnd3 = random.Random(7)
            e3, tm3, route3, _ = timed_steps(f3, _lib, P2, L2, K2, W2, s2, synthetic_controls(K2 + W2),
                                              [rnd3.random() for _ in range(K2 + W2)], None, barrier2(torch, f3), 4)
            if route3 in ("ml_regs", "ml_fused") and f3.observe_published():
                route3 += "_pub"
            second["k_step_fused"] = {"what": "the same workload with the option pub_small = 0: k_step_fused, the default of rounds 1-5", "ms_per_step": e3 / K2 * 1e3,
                                      "value": float(P2) * L2 * K2 / e3,
                                      "roofline": roofline_object(P2, L2, route3, tm3["observe"][0], tm3["observe"][1], 4, K2, None)}
            f3.close()
            del f3
        except Exception as e:  # noqa: BLE001
            second["k_step_fused"] = {"error": repr(e)}

    # One whole shard of BASELINE.json configs[4] (1 000 000 x 5 000 over 8 GPUs = 125 000 x 5 000 per GPU) on this GPU: the two-pass
    # kernel k_step_pub_big, timed by the driver's run and not only in profiles/ (N = 1, default workload only)
    shard4 = None
    if world == 1 and not args.force_sharded and not args.no_configs4 and (P, L) == (DEFAULT_P, DEFAULT_L) and args.assoc == "ml":
        # (round 5: the same window of the trajectory as the headline -- warm-up 5, 20 steps -- where rounds 3-4 timed steps 2-7
        # of the fresh filter; and the steps 40-49 beside it: the map's colour blocks tighten for some twenty steps, and with
        # them the scan-level pruning of look-alikes)
        P4, L4, K4, W4, LATE0, LATEK = 125000, 5000, 20, 5, 40, 10
        f4 = None
        try:
            n4 = LATE0 + LATEK
            m4, c4, s4 = synthetic_inputs(L4, n4)
            ws4 = synthetic_controls(n4)
            f4 = _lib.DeviceFilter(P4, L4, device=local_rank)
            env_options(f4)
            f4.upload_map(m4, c4.reshape(L4, 25))
            rnd4 = random.Random(7)
            us4 = [rnd4.random() for _ in range(n4)]
            e4, tm4, route4, step4 = timed_steps(f4, _lib, P4, L4, K4, W4, s4, ws4, us4, None, barrier2(torch, f4), 1)
            warm4 = {"ms": [round(v, 3) for v in timed_steps.warmup_ms], "flagged_particles": list(timed_steps.warmup_flagged)}
            fl4 = f4.observe_flagged()
            for s_ in range(W4 + K4, LATE0):
                step4(s_)
            f4.synchronize()
            f4.enable_timing(0b0000100)
            f4.reset_timings()
            t_l = time.perf_counter()
            for s_ in range(LATE0, LATE0 + LATEK):
                step4(s_)
            f4.synchronize()
            e_late = time.perf_counter() - t_l
            tl4 = f4.timings()["observe"]
            f4.enable_timing(0)
            shard4 = {
                "workload": workload_name(P4, L4, "ml"),
                "value": float(P4) * L4 * K4 / e4,
                "unit": "updates/s",
                "steps": K4,
                "warmup": W4,
                "ms_per_step": e4 / K4 * 1e3,
                "filter_steps_per_sec": K4 / e4,
                "device_bytes": f4.device_bytes(),
                "particles_sent_to_fallback_kernels_last_step": fl4[0],
                "trajectory_steps": [W4, W4 + K4 - 1],
                "warmup_steps": warm4,  # step 0, the first scan of the fresh map, is the slowest of the run (99 ms in round 5)
                "roofline": roofline_object(P4, L4, route4, tm4["observe"][0], tm4["observe"][1], 1, K4, None),
                "late_window": {"trajectory_steps": [LATE0, LATE0 + LATEK - 1], "ms_per_step": e_late / LATEK * 1e3,
                                "roofline": roofline_object(P4, L4, route4, tl4[0], tl4[1], 1, LATEK, None)},
            }
        except Exception as e:  # (a GPU with less free memory than 170 GB: say so instead of failing the headline)
            shard4 = {"workload": workload_name(P4, L4, "ml"), "error": repr(e)}
        finally:  # (170 GB must not stay allocated behind a failure while the rest of the line is measured)
            if f4 is not None:
                f4.close()
            f4 = None

    # The reference's own scene sizes through the FACADE (FastSLAM.cam_cb wall time, Python included): prkt_ros.py's node --
    # 50 particles x 4 landmarks (prkt_ros.py:33-52; mutable, as BASELINE.md section 2 measured them) -- and BASELINE configs[0],
    # 100 x 50.  BASELINE.md section 2 holds the reference's own figures for the same sizes (build container, one CPU core).
    refscene = None
    if world == 1 and not args.force_sharded and not args.no_refscene and (P, L) == (DEFAULT_P, DEFAULT_L) and args.assoc == "ml":
        refscene = facade_latency(local_rank)
        try:  # the reference's call pattern at the headline's size
            refscene["configs2_through_the_facade"] = facade_at_size(local_rank, DEFAULT_P, DEFAULT_L, 20, 5)
        except Exception as e:  # noqa: BLE001
            refscene["configs2_through_the_facade"] = {"error": repr(e)}
        try:  # SURVEY 8 row (f4) at device speed: maps that grow, the per-particle bookkeeping on the device
            refscene["new_landmarks"] = facade_growing(local_rank, 10000, 40, 6, 12)
        except Exception as e:  # noqa: BLE001
            refscene["new_landmarks"] = {"error": repr(e)}
        try:  # ... and at the headline's size: 100 000 particles, 2 000 preset + 6 unknown landmarks, 16 spare slots
            g = facade_growing(local_rank, DEFAULT_P, DEFAULT_L, 6, 14, spare=16)
            fixed = (refscene.get("configs2_through_the_facade") or {}).get("array", {}).get("ms_per_step")
            g["fixed_map_ms_per_step"] = fixed
            if fixed and g.get("ms_per_step_afterwards"):
                g["afterwards_over_fixed_map"] = g["ms_per_step_afterwards"] / fixed
            refscene["new_landmarks_at_scale"] = g
        except Exception as e:  # noqa: BLE001
            refscene["new_landmarks_at_scale"] = {"error": repr(e)}

    # what a plain device-to-device copy reaches on THIS box (read + write bytes / time), outside the
    # timed region: the practical ceiling next to the 8 TB/s vendor figure
    copy_gbs = None
    if rank == 0 and args.full:
        n = 1 << 27  # 2 x 1 GiB of float64
        a = torch.empty(n, dtype=torch.float64, device="cuda").normal_()
        b = torch.empty_like(a)
        for _ in range(3):
            b.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        copy_gbs = 2.0 * 8 * n * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        del a, b

    if world > 1:
        import torch.distributed as dist

        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    backend_name = "none"
    rank_devices = None
    if sharded:
        import torch.distributed as dist

        backend_name = "%s%s" % (dist.get_backend(), " (= RCCL over xGMI)" if dist.get_backend() == "nccl" else "")
        # which physical device every rank really ran on (so that a SCALE record can be checked for "N ranks on N GPUs")
        prop = torch.cuda.get_device_properties(local_rank)
        mine = {"rank": rank, "device_index": local_rank, "name": prop.name,
                "uuid": str(getattr(prop, "uuid", "")), "pci_bus_id": getattr(prop, "pci_bus_id", None)}
        if world > 1:
            rank_devices = [None] * world
            dist.all_gather_object(rank_devices, mine)
        else:
            rank_devices = [mine]
    n_devices = world
    if rank_devices is not None:
        n_devices = len(set((d["uuid"], d["pci_bus_id"], d["device_index"]) for d in rank_devices))
    if rank == 0:
        total_updates = float(P) * world * L * K
        obs_ms, obs_n = tm["observe"]
        assoc_ms, assoc_n = tm["assoc"]
        roof = roofline_object(P, L, route, obs_ms, obs_n, stride, K, copy_gbs)
        obs_avg_s = (obs_ms / max(obs_n, 1)) * 1e-3
        if uniq and obs_avg_s > 0:
            mean_unique = float(np.mean(uniq))
            half = float(L) * BYTES_PER_UPDATE / 2.0
            roof["unique_source_slots"] = mean_unique
            roof["unique_source_slots_note"] = "distinct map slots read by one observe launch (of %d particles), mean of %d " \
                "untimed steps behind the timed region" % (P, len(uniq))
            roof["achieved_unique"] = (mean_unique * half + float(P) * half) / obs_avg_s / 1e9
            roof["frac_unique"] = roof["achieved_unique"] / HBM_PEAK_GBS
        if no_dup and args.assoc in no_dup:
            roof["frac_no_duplicates"] = no_dup[args.assoc]["frac"]
        elif no_dup and args.assoc == "known":
            roof["frac_no_duplicates"] = no_dup["supplied_ids"]["frac"]
        if no_dup:
            roof["no_resample_probe"] = no_dup
        if known is not None:
            roof["ekf_stage"] = known
        if args.full:  # (the association kernel is timed in the untimed steps behind the timed region)
            roof["assoc_kernel_ms"] = assoc_ms / max(assoc_n, 1)
        if flagged is not None:
            roof["particles_sent_to_general_kernels_last_step"] = flagged[0]
            roof["candidate_list_overflows_last_step"] = flagged[1]
        if second is not None and copy_gbs:
            second["roofline"]["copy_measured"] = copy_gbs
            second["roofline"]["frac_of_copy"] = second["roofline"]["achieved"] / copy_gbs
        out = {
            "metric": "particle*landmark EKF updates/sec (whole filter step)",
            "value": total_updates / elapsed,
            "unit": "updates/s",
            "n_gpus": n_devices,
            "steps": K,
            "warmup": W,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "filter_steps_per_sec": K / elapsed,
            "config": {
                "workload": workload_name(P, L, args.assoc),
                "particles_per_gpu": P,
                "landmarks": L,
                "blobs": L,
                "assoc": args.assoc,
                "global_particles": P * world,
                "parallelism": "particles sharded over %d rank(s) on %d GPU(s), one process per GPU; backend %s: all-reduce(max) + "
                "all-gather(block weight totals) + all-to-all(migrating particles) per resample" % (world, n_devices, backend_name) if sharded
                else "single GPU",
            },
            "roofline": roof,
            "kernel_ms_per_step": {"observe": obs_ms / max(obs_n, 1), "assoc": assoc_ms / max(assoc_n, 1)} if args.full
            else {"observe": obs_ms / max(obs_n, 1)},
            "summary": list(summary),
            "matched_fraction_last_timed_scan": matched,  # validity: the scans stayed matchable to the end
        }
        if head_warm is not None:
            out["warmup_steps"] = head_warm
        if replay is not None:
            out["per_step"] = replay
            kmm = replay.get("kernel_ms_min_max_timed_window")
            if kmm and kmm[0] > 0:
                # the kernel's slowest and fastest launch over the timed window's trajectory steps (the untimed replay, every step
                # bracketed): the fraction drifts across a run as the particle cloud converges
                alg = float(P) * L * BYTES_PER_UPDATE / 1e9
                roof["frac_range_over_steps"] = [alg / (kmm[1] * 1e-3) / HBM_PEAK_GBS, alg / (kmm[0] * 1e-3) / HBM_PEAK_GBS]
            if replay.get("slow_window"):
                out["slow_window_ms_per_step"] = replay["slow_window"]["ms_mean"]
        if sharded:
            out["world_size"] = world  # dist.get_world_size(): the ranks the process group really formed
            out["rank_devices"] = rank_devices
            if same_gpu or n_devices != world:
                out["rehearsal"] = True  # several ranks share a device: control flow only, NOT a scaling measurement
                out["rehearsal_note"] = "%d ranks on %d device(s) over %s: the value is not a multi-GPU throughput" % (world, n_devices, backend_name)
        if migrated is not None:
            out["placement"] = placement  # "balanced": only a rank's excess children travel, only particles that have any
            out["migrated_particles_per_step"] = migrated  # all ranks together: each one is a pose + a whole map slot on the wire
            out["migrated_bytes_per_step"] = migrated_bytes
        if second is not None:
            out["configs1"] = second
        if shard4 is not None:
            out["configs4_shard"] = shard4
        if refscene is not None:
            out["refscene"] = refscene
        if cpu is not None:
            out["cpu_baseline"] = cpu
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    elif args.force_sharded:  # (the single-rank group of --force-sharded)
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()


def facade_at_size(device, P, L, steps, warm):
    """FastSLAM.cam_cb + summary() per step -- what prkt_ros.py:84-85 does: the summary synchronises every step -- at a BASELINE
    size, through the facade (device RNG, log weights: the throughput mode; the association, the EKF and the resample are the
    same kernels as in the headline).  Three ways of handing the scan over: message objects (the reference's interface:
    ros_view.last_sensor_reading.observes, 4 attribute reads per blob), the same scan object again (a ROS node whose camera is
    slower than its 10 Hz loop sees that: prkt_ros.py:109 keeps the last message), and a (B, 4) array."""
    import parakeet_slam_amd as pk

    class Scan(object):
        pass

    class Node(object):
        pass

    means, covs, scans = synthetic_inputs(L, steps + warm)
    ws = synthetic_controls(steps + warm)
    feats = [pk.Feature(mean=means[l], covar=covs[l]) for l in range(L)]
    out = {"what": "wall time of FastSLAM.cam_cb + FastSLAM.summary() per step (the reference's call pattern, prkt_ros.py:84-85: one "
                   "synchronisation per step), %d particles x %d landmarks, B = L, rng='device', weights 'log'; steps %d..%d of the "
                   "trajectory" % (P, L, warm, warm + steps - 1)}

    def blobs_of(sc):
        obs = []
        for b in sc:
            o = pk.msgs.Blob()
            o.bearing = float(b[0])
            o.color.r, o.color.g, o.color.b = float(b[1]), float(b[2]), float(b[3])
            obs.append(o)
        return obs

    for tag in ("message_objects", "array"):
        views = [blobs_of(sc) for sc in scans] if tag == "message_objects" else [np.ascontiguousarray(sc) for sc in scans]
        pk.msgs.Time.set_now(0.0)
        random.seed(7)
        fs = pk.FastSLAM(feats, num_particles=P, device=device, weight_domain="log", rng="device", seed=7)
        node = Node()
        node.last_sensor_reading = Scan()
        t = 0.0
        dts = []
        for s_ in range(warm + steps):
            tw = pk.msgs.Twist()
            tw.linear.x, tw.angular.z = 0.2, ws[s_]
            fs.last_control = tw
            t += 0.1
            pk.msgs.Time.set_now(t)
            node.last_sensor_reading.observes = views[s_]
            t0 = time.perf_counter()
            fs.cam_cb(node)
            sm = fs.summary()
            dts.append(time.perf_counter() - t0)
        fs.close()
        d = np.array(dts[warm:])
        out[tag] = {"ms_per_step": float(d.mean() * 1e3), "ms_p95": float(np.percentile(d, 95) * 1e3), "ms_max": float(d.max() * 1e3),
                    "steps": steps, "summary": [float(v) for v in sm]}
    return out


def facade_growing(device, P, L0, U, steps, spare=None):
    """FastSLAM(new_landmarks=True).cam_cb + summary() per step on a scene with U landmarks the preset map does not hold
    (prkt_core_v2.py:546-746 made to work): the unmatched blobs of every particle are paired and
    triangulated by ONE kernel behind the observe, the readings / id counters / slot ids live in HBM and follow the resample on
    the device.  Nothing per particle crosses to the host inside a step."""
    import parakeet_slam_amd as pk

    class Scan(object):
        pass

    class Node(object):
        pass

    means, covs, _ = synthetic_inputs(L0 + U, 1)
    feats = [pk.Feature(mean=means[l], covar=covs[l]) for l in range(L0)]
    pk.msgs.Time.set_now(0.0)
    random.seed(7)
    fs = pk.FastSLAM(feats, num_particles=P, device=device, weight_domain="log", rng="device", seed=7, new_landmarks=True,
                     spare_landmarks=(U + 2) if spare is None else spare, publish_debug=False)
    node = Node()
    node.last_sensor_reading = Scan()
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = 0.5, 0.2
    fs.last_control = tw
    pose, dts, used = (0.0, 0.0, 0.0), [], []
    for s_ in range(steps):
        h1 = pose[2] + 0.2 * 0.1
        pose = (pose[0] + 0.1 * math.cos(h1), pose[1] + 0.1 * math.sin(h1), pose[2] + 0.04)  # v = 0.5, w = 0.2, dt = 0.2, no noise
        pk.msgs.Time.set_now(0.2 * (s_ + 1))
        b = np.empty((L0 + U, 4))
        b[:, 0] = np.arctan2(means[:, 1] - pose[1], means[:, 0] - pose[0]) - pose[2]
        b[:, 1:] = means[:, 2:]
        node.last_sensor_reading.observes = b
        t0 = time.perf_counter()
        fs.cam_cb(node)
        fs.summary()
        dts.append(time.perf_counter() - t0)
        used.append(float(fs._filter.grow_download(readings=False, slot_ids=False)[0][:, 1].mean()))  # (the bench's own look at the counters: outside the timed step)
    k = fs._filter.download_landmarks(means=False, covs=False)[2][:, L0:]
    u = fs._filter.grow_download(readings=False, slot_ids=False)[0][:, 1]
    promoted = float((((k & 0x40000000) == 0) & (np.arange(k.shape[1])[None, :] < u[:, None])).sum() / float(P))
    growing = [i for i in range(1, steps) if used[i] > used[i - 1]]
    out = {"what": "wall time of FastSLAM(new_landmarks=True).cam_cb + summary() per step, %d particles, %d preset + %d unknown landmarks, "
                   "bookkeeping='device' (pk_k_grow.hip); since round 6 on the one-pass route of the map's size (the publish / subscribe kernels leave "
                   "every particle's unmatched blobs as a bit row; rounds 2-5: the general route, whose ids the bookkeeping kernel read)" % (P, L0, U),
           "route": fs._filter.observe_route(), "one_pass_kernel_did_the_last_scan": bool(fs._filter.observe_published()),
           "particles_sent_to_general_kernels_last_step": int(fs._filter.observe_flagged()[0]),
           "ms_per_step": [round(x * 1e3, 3) for x in dts],
           "ms_per_step_while_maps_grow": round(float(np.mean([dts[i] for i in growing])) * 1e3, 3) if growing else None,
           "ms_per_step_afterwards": round(float(np.mean(dts[max(growing) + 1:])) * 1e3, 3) if growing and max(growing) + 1 < steps else None,
           "spare_slots_in_use_mean": used, "promoted_per_particle": promoted, "readings_dropped": fs.readings_dropped(),
           "host_loop_note": "the same scene with bookkeeping='host' (rounds 2-4): 90-900 ms per growing step (profiles/r05/grow_speed_10000x40.json)"}
    fs.close()
    return out


def facade_latency(device):
    """cam_cb through parakeet_slam_amd.FastSLAM at the reference's own sizes: seconds per filter step, host side included."""
    import parakeet_slam_amd as pk

    class Scan(object):
        pass

    class Node(object):
        pass

    out = {"what": "wall time of FastSLAM.cam_cb (facade + C ABI + kernels, one synchronising summary() per step as prkt_ros.py:84-85 "
                   "does), rng='global', weights 'linear' -- the reference's semantics",
           "reference_note": "BASELINE.md section 2: the unmodified reference takes 0.135 s per step at 50 x 4 (author's profile) and "
                             "7.86 s per step at 100 x 50 (measured in the build container, 1 core)"}
    for tag, P, L, immutable, steps, ref_s in (("prkt_ros_size_50x4", 50, 4, False, 200, 0.135), ("configs0_100x50", 100, 50, False, 100, 7.86)):
        means, covs, scans = synthetic_inputs(L, steps + 5)
        feats = []
        for l in range(L):
            f = pk.Feature(mean=means[l], covar=covs[l])
            f.__immutable__ = immutable
            feats.append(f)
        pk.msgs.Time.set_now(0.0)
        np.random.seed(7)
        random.seed(7)
        fs = pk.FastSLAM(feats, num_particles=P, device=device)
        tw = pk.msgs.Twist()
        tw.linear.x, tw.angular.z = 0.2, 0.1
        fs.last_control = tw
        node = Node()
        node.last_sensor_reading = Scan()
        t = 0.0

        def blobs_of(sc):
            obs = []
            for b in sc:
                o = pk.msgs.Blob()
                o.bearing = float(b[0])
                o.color.r, o.color.g, o.color.b = float(b[1]), float(b[2]), float(b[3])
                obs.append(o)
            return obs

        views = [blobs_of(sc) for sc in scans]
        for s_ in range(5):
            t += 0.1
            pk.msgs.Time.set_now(t)
            node.last_sensor_reading.observes = views[s_]
            fs.cam_cb(node)
            fs.summary()
        t0 = time.perf_counter()
        for s_ in range(5, 5 + steps):
            t += 0.1
            pk.msgs.Time.set_now(t)
            node.last_sensor_reading.observes = views[s_]
            fs.cam_cb(node)
            fs.summary()
        dt = (time.perf_counter() - t0) / steps
        fs.close()
        out[tag] = {"particles": P, "landmarks": L, "blobs": L, "immutable_landmarks": immutable, "steps": steps,
                    "seconds_per_step": dt, "steps_per_sec": 1.0 / dt, "reference_seconds_per_step": ref_s,
                    "reference_source": "BASELINE.md section 2 (measured in the build container / the author's profile; not on this box)",
                    "speedup_vs_reference": ref_s / dt}
    pk.msgs.Time.set_now(None)
    return out


def barrier2(torch, filt):
    def b():
        torch.cuda.synchronize()
        filt.synchronize()
    return b


if __name__ == "__main__":
    main()

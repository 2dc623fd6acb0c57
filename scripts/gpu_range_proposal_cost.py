"""What ranges in the measurement-informed proposal cost (pk_proposal_ranges; DESIGN.md section 4, "Ranges in the proposal") on one
GPU, in the manner of scripts/gpu_proposal_cost.py: bearing-model filters of 10 000 x 500 and 100 000 x 2 000 on synthetic_world(L),
blob j seeing landmark j from a slow drive, a fresh filter per run, three variants alternating in one call, three runs each:
  bearing-only          pk_propose(fresh) + pk_resample on scans without ranges (k_assoc_grid_bearing, k_propose, k_observe_proposed)
  all ranged            the same with a range on every blob (k_assoc_grid_range, k_propose_range, k_observe_proposed_range)
  every third unranged  ... and with blobs 2, 5, 8, ... unranged: the same kernels, both paths in every wave
Per run: WARM untimed steps, then STEPS steps between two synchronisations on the host clock -> ms per step, and the same steps on
another fresh filter with pk_enable_timing on -> ms per step of the association, k_propose(_range) and the observe, n_eff / P in front
of every resample.  Then ONE rocprofv3 --kernel-trace run of its own (a child process; 10 000 x 500 only) for the per-kernel times
behind those spans.  One JSON line per run, one summary line per shape, one line per traced kernel.
    python scripts/gpu_range_proposal_cost.py [--out FILE] [--steps N] [--shapes PxL,PxL] [--no-trace]"""
import csv
import glob
import json
import math
import os
import random
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle.fastslam_oracle import synthetic_world, truth_step  # noqa: E402
from parakeet_slam_amd import _lib  # noqa: E402

LOG = _lib.PK_WEIGHTS_LOG
WARM = 3
VARIANTS = ("bearing-only", "all ranged", "every third unranged")
SPANS = ("motion", "assoc", "propose", "observe", "resample")
KERNELS = ("k_assoc_grid_bearing", "k_assoc_grid_range", "k_propose", "k_propose_range", "k_observe_proposed", "k_observe_proposed_range")
V, W, DT = 0.2, 0.1, 0.1
SIGMA_B, SIGMA_C, SIGMA_R = 0.01, 0.3, (0.05, 0.01)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def wrap(a):
    return a - 2.0 * math.pi * np.rint(a / (2.0 * math.pi))


def scans_of(world, n):
    """The drive's scans, blob j seeing landmark j: per step (blobs, noisy ranges, their variances)."""
    rs, rr = np.random.RandomState(1), np.random.RandomState(2)
    pose, L, out = (0.0, 0.0, 0.0), len(world), []
    for _ in range(n):
        pose = truth_step(pose, V, W, DT)
        x, y, h = pose
        blobs = np.empty((L, 4))
        blobs[:, 0] = wrap(np.arctan2(world[:, 1] - y, world[:, 0] - x) - h + SIGMA_B * rs.standard_normal(L))
        blobs[:, 1:] = world[:, 2:] + SIGMA_C * rs.standard_normal((L, 3))
        rho = np.hypot(world[:, 0] - x, world[:, 1] - y)
        rho = np.maximum(rho + (SIGMA_R[0] + SIGMA_R[1] * rho) * rr.standard_normal(L), 1e-3)
        out.append((blobs, rho, (SIGMA_R[0] + SIGMA_R[1] * rho) ** 2))
    return out


def drive(P, L, variant, world, covs, scans, steps, timed):
    f = _lib.DeviceFilter(P, L)
    f.set_measurement_model("bearing")
    f.proposal_ranges(True)
    f.upload_map(world, covs.reshape(L, 25))
    rnd = random.Random(7)
    s = 0
    neff = []

    def run(n, measure):
        nonlocal s
        for _ in range(n):
            blobs, rho, var = scans[s]
            if variant != "bearing-only":
                if variant == "every third unranged":
                    rho = rho.copy()
                    rho[2::3] = np.nan
                f.scan_ranges(rho, var)
            f.propose(V, W, DT, blobs, seed=7, draw=s, fresh=True)
            if measure:
                neff.append(f.n_eff(LOG) / P)
            f.resample(rnd.random(), domain=LOG)
            s += 1
        f.synchronize()

    run(WARM, False)
    if timed:
        f.enable_timing(-1)
        f.reset_timings()
    t0 = time.perf_counter()
    run(steps, timed)
    ms_step = (time.perf_counter() - t0) * 1e3 / steps
    out = (ms_step, f.observe_route(), f.timings() if timed else None, f.summary(), neff)
    f.close()
    return out


def one_run(P, L, variant, world, covs, scans, steps):
    ms_step, route, _, summary, _ = drive(P, L, variant, world, covs, scans, steps, False)
    _, _, t, again, neff = drive(P, L, variant, world, covs, scans, steps, True)  # the SAME steps, bracketed by events
    assert again == summary, (again, summary)
    out = dict(route=route, ms_per_step=round(ms_step, 4), n_eff_over_P=round(sum(neff) / len(neff), 4), summary=summary)
    for k in SPANS:
        out[k + "_ms_per_step"] = round(t[k][0] / steps, 4)
        out[k + "_launches_per_step"] = t[k][1] / steps
    return out


def trace_child(P, L, steps):
    world, covs = synthetic_world(L, seed=5)
    scans = scans_of(world, len(VARIANTS) * (WARM + steps))
    for i, variant in enumerate(VARIANTS):
        drive(P, L, variant, world, covs, scans[i * (WARM + steps):], steps, False)


def kernel_trace(P, L, steps, work):
    """{kernel: microseconds of its launches}, in launch order, from one rocprofv3 --kernel-trace run of a child process."""
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", work, "--", sys.executable, os.path.abspath(__file__), "--trace",
           "--steps", str(steps), "--shapes", "%dx%d" % (P, L)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=280)
    rows = []
    for path in glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {k: [] for k in KERNELS}
    for r in rows:
        name = r["Kernel_Name"]
        for k in sorted(KERNELS, key=len, reverse=True):  # (the longest name that fits: k_propose_range before k_propose)
            if k + "<" in name or k + "(" in name or name.endswith(k):
                out[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    return out


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


if __name__ == "__main__":
    out_path = arg("--out", os.path.join("out", "range_proposal_cost.json"))
    steps = int(arg("--steps", "10"))
    shapes = [tuple(int(x) for x in sh.split("x")) for sh in arg("--shapes", "10000x500,100000x2000").split(",")]
    if "--trace" in sys.argv:
        trace_child(shapes[0][0], shapes[0][1], steps)
        sys.exit(0)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)

    for P, L in shapes:
        world, covs = synthetic_world(L, seed=5)
        scans = scans_of(world, WARM + steps)
        runs = {name: [] for name in VARIANTS}
        for repeat in (1, 2, 3):
            for name in VARIANTS:  # alternating
                r = one_run(P, L, name, world, covs, scans, steps)
                runs[name].append(r)
                emit(dict(what="run", particles=P, landmarks=L, blobs=L, variant=name, repeat=repeat, steps=steps, **r))
        keys = ["ms_per_step", "n_eff_over_P"] + [k + "_ms_per_step" for k in SPANS]
        med = {name: {k: median([r[k] for r in rs]) for k in keys} for name, rs in runs.items()}
        spread = {name: round((max(r["ms_per_step"] for r in rs) - min(r["ms_per_step"] for r in rs)) / med[name]["ms_per_step"], 4)
                  for name, rs in runs.items()}
        base = med["bearing-only"]["ms_per_step"]
        emit(dict(what="medians of three", particles=P, landmarks=L, medians=med, spread_of_ms_per_step=spread,
                  step_over_bearing_only={name: round(med[name]["ms_per_step"] / base, 4) for name in VARIANTS}))
    if "--no-trace" not in sys.argv:
        P, L = shapes[0]
        t = kernel_trace(P, L, steps, os.path.join(os.path.dirname(out_path) or ".", "range_proposal_trace"))
        n = WARM + steps
        for k in KERNELS:
            # the range instances ran the second and the third variant, in that order; the warm-up launches of each are dropped
            parts = ({VARIANTS[1]: t[k][WARM:n], VARIANTS[2]: t[k][n + WARM:]} if k.endswith("_range") and len(t[k]) == 2 * n
                     else {VARIANTS[0]: t[k][WARM:]})
            for variant, v in parts.items():
                if v:
                    emit(dict(what="kernel trace, us per launch", particles=P, landmarks=L, kernel=k, variant=variant, launches=len(v),
                              median=round(median(v), 2), min=round(min(v), 2), max=round(max(v), 2)))
    fh.close()

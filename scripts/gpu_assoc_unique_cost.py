"""What unique association costs (pk_assoc_unique; DESIGN.md section 4, "Unique association") on one GPU, by pk_enable_timing.
  1. the PK_T_ASSOC time of a bearing-model scan at the configs[1] and configs[2] shapes with the mode on against the general route
     with the mode off (the kernels every commit before this one ran: the mode off launches nothing else), on the benchmark's
     trajectory, where conflicts are rare: ONE filter per shape drives the same WARM + STEPS steps again and again from the same
     start, the mode alternating drive by drive, RUNS drives each; the added microseconds per scan, and the share of particles
     that left k_assoc_unique after its first pass (pk_assoc_unique_stats).
  2. the same filter on a scan built to conflict in every particle (landmarks whose colours come in clusters, every blob one of
     several that show the same landmark): the time and the counters.
One JSON line per figure.
    python scripts/gpu_assoc_unique_cost.py [--out FILE] [--steps N] [--runs N] [--shapes 10000x500,100000x2000]"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bench import synthetic_inputs  # noqa: E402

WARM = 3
T_ASSOC = 1  # PK_T_ASSOC


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def wrap(a):
    return a - 2.0 * np.pi * np.rint(a / (2.0 * np.pi))


def clustered(L, B, seed=3):
    """A map whose colours come in clusters of about eight, in the front sector, and B blobs that show landmarks of its first half."""
    rs = np.random.RandomState(seed)
    phi, rho = rs.uniform(-1.3, 1.3, L), rs.uniform(8.0, 30.0, L)
    centres = rs.uniform(30.0, 225.0, (max(1, L // 8), 3))
    means = np.empty((L, 5))
    means[:, 0], means[:, 1] = rho * np.cos(phi), rho * np.sin(phi)
    means[:, 2:] = centres[rs.randint(len(centres), size=L)] + rs.uniform(-5.0, 5.0, (L, 3))
    covs = np.broadcast_to(np.diag([1.0, 1.0, 4.0, 4.0, 4.0]), (L, 5, 5)).copy()
    j = rs.randint(0, L // 2, B)
    blobs = np.empty((B, 4))
    blobs[:, 0] = np.arctan2(means[j, 1], means[j, 0]) + 0.02 * rs.standard_normal(B)
    blobs[:, 1:] = means[j, 2:] + rs.standard_normal((B, 3))
    return means, covs, blobs


def drive(lib, f, means, covs, scans, steps, on, warm=WARM):
    """One drive from the start: per measured step the PK_T_ASSOC milliseconds and the mode's counters."""
    P, L = f.P, f.L
    f.upload_map(means, covs.reshape(L, 25))
    xyhw = np.zeros((P, 4))
    xyhw[:, 3] = 1.0
    f.upload_poses(xyhw)
    f.assoc_unique(on)
    ms, stats = [], []
    for s in range(warm + steps):
        f.motion(0.2, 0.1, 0.1, seed=7, draw=s)
        f.reset_timings()
        f.observe(scans[s], fresh=True)
        assert f.observe_route() == "ml_general"
        t = f.timings()["assoc"][0]
        f.resample(0.5, domain=lib.PK_WEIGHTS_LOG)
        if s >= warm:
            ms.append(float(t))
            stats.append([int(v) for v in f.assoc_unique_stats()])
    return ms, stats


if __name__ == "__main__":
    from parakeet_slam_amd import _lib as lib

    steps, runs = int(arg("--steps", "5")), int(arg("--runs", "3"))
    shapes = [tuple(int(v) for v in s.split("x")) for s in arg("--shapes", "10000x500,100000x2000").split(",")]
    out_path = arg("--out", os.path.join("out", "assoc_unique_cost.json"))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)

    med = lambda v: float(np.median(v))
    for P, L in shapes:
        f = lib.DeviceFilter(P, L)
        f.set_measurement_model("bearing")
        f.enable_timing(1 << T_ASSOC)
        means, covs, scans = synthetic_inputs(L, WARM + steps)
        scans = [np.column_stack([wrap(b[:, 0]), b[:, 1:]]) for b in scans]
        per = {False: [], True: []}
        left = []
        for r in range(runs):
            for on in (False, True):
                ms, stats = drive(lib, f, means, covs, scans, steps, on)
                per[on].append(ms)
                if on:
                    left += [1.0 - st[0] / float(P) for st in stats]
                    last = stats[-1]
        off_us, on_us = 1e3 * np.array(per[False]), 1e3 * np.array(per[True])
        emit(dict(what="PK_T_ASSOC per scan on the benchmark's trajectory, bearing model, general route", particles=P, landmarks=L, blobs=L,
                  runs=runs, steps=steps, off_us_median=round(med(off_us), 1), off_us_min=round(float(off_us.min()), 1),
                  off_us_max=round(float(off_us.max()), 1), on_us_median=round(med(on_us), 1), on_us_min=round(float(on_us.min()), 1),
                  on_us_max=round(float(on_us.max()), 1), added_us_median_of_step_medians=round(med(np.median(on_us, axis=0) - np.median(off_us, axis=0)), 1),
                  share_left_after_first_pass_min=round(min(left), 5), share_left_after_first_pass_mean=round(float(np.mean(left)), 5),
                  last_scan_stats=last))
        # a scan built to conflict in every particle
        cm, cc, cb = clustered(L, L)
        per = {False: [], True: []}
        for r in range(runs):
            for on in (False, True):
                ms, stats = drive(lib, f, cm, cc, [cb], 1, on, warm=0)
                per[on].append(ms[0])
                if on:
                    last = stats[-1]
        emit(dict(what="PK_T_ASSOC of a scan built to conflict in every particle (the first scan on the uploaded map)", particles=P, landmarks=L,
                  blobs=L, runs=runs, off_us=[round(1e3 * v, 1) for v in per[False]], on_us=[round(1e3 * v, 1) for v in per[True]],
                  stats_conflicts_changed_rematched_passes=last))
        f.close()
    fh.close()

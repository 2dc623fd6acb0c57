"""What range-bearing scans cost and buy (pk_scan_ranges; DESIGN.md section 4, "Range-bearing scans") on one GPU.
  1. before this process opens the GPU: `rocprofv3 --kernel-trace` (a run of its own, no counters) over a child (--trace) that steps a
     10 000 x 500 bearing-model filter through scans of 500 blobs: WARM steps, then STEPS steps each of scans with no range
     (k_assoc_grid_bearing + k_observe_bearing, today's instances), with a range on every blob and with every third blob unranged
     (k_assoc_grid_range + k_observe_range both).  The launches of the association and observe kernels are taken from the trace in
     launch order, STEPS per kind: time per launch (median, min, max) and the ratio to today's instances.
  2. the accuracy table of tests/test_range_bearing_host.py through the device facade: the turning drive (64 particles, 12
     landmarks, 40 steps) with the map's starting positions pushed 0.5 m off, seeds 1-3, FastSLAM(measurement_model="bearing") with
     and without range_noise=(0.05, 0.01): the landmarks' mean distance from the truth, the pose error (mean, max).
One JSON line per figure.
    python scripts/gpu_range_scan_cost.py [--out FILE] [--steps N]"""
import csv
import glob
import json
import math
import os
import random
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle.fastslam_oracle import synthetic_world, truth_step  # noqa: E402

P, L, WARM = 10000, 500, 3
KINDS = ("none", "all", "every third unranged")
V, W, DT = 1.0, 0.35, 0.5
SIGMA_B, SIGMA_C, SIGMA_R = 0.01, 0.3, (0.05, 0.01)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def wrap(a):
    return a - 2.0 * math.pi * np.rint(a / (2.0 * math.pi))


def scan_of(world, pose, rs, rr):
    """Blob j sees landmark j: (bearing, r, g, b) with the drive's noise, wrapped; the noisy ranges and their variances."""
    x, y, h = pose
    n = len(world)
    blobs = np.empty((n, 4))
    blobs[:, 0] = wrap(np.arctan2(world[:, 1] - y, world[:, 0] - x) - h + SIGMA_B * rs.standard_normal(n))
    blobs[:, 1:] = world[:, 2:] + SIGMA_C * rs.standard_normal((n, 3))
    rho = np.hypot(world[:, 0] - x, world[:, 1] - y)
    rho = rho + (SIGMA_R[0] + SIGMA_R[1] * rho) * rr.standard_normal(n)
    return blobs, rho, (SIGMA_R[0] + SIGMA_R[1] * rho) ** 2


def trace_child(steps):
    from parakeet_slam_amd import _lib

    world, covs = synthetic_world(L, seed=5)
    f = _lib.DeviceFilter(P, L)
    f.set_measurement_model("bearing")
    f.upload_map(world, covs.reshape(L, 25))
    rs, rr, rnd = np.random.RandomState(1), np.random.RandomState(2), random.Random(7)
    pose = (0.0, 0.0, 0.0)
    s = 0
    for kind in ("warm",) + KINDS:
        for _ in range(WARM if kind == "warm" else steps):
            pose = truth_step(pose, 0.2, 0.1, 0.1)
            blobs, rho, var = scan_of(world, pose, rs, rr)
            if kind == "every third unranged":
                rho[2::3] = np.nan
            if kind in KINDS[1:]:
                f.scan_ranges(rho, var)
            f.step(0.2, 0.1, 0.1, blobs, rnd.random(), seed=7, draw=s, domain=_lib.PK_WEIGHTS_LOG)
            assert f.observe_route() == "ml_general"
            s += 1
    f.synchronize()
    f.close()


def kernel_trace(steps, work):
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", work, "--", sys.executable, os.path.abspath(__file__), "--trace",
           "--steps", str(steps)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=280)
    rows = []
    for path in glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for stage, today, ranged in (("assoc", "k_assoc_grid_bearing", "k_assoc_grid_range"), ("observe", "k_observe_bearing", "k_observe_range")):
        us = lambda name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        a, b = us(today), us(ranged)
        assert len(a) == WARM + steps and len(b) == 2 * steps, (stage, len(a), len(b))
        out[stage] = {KINDS[0]: a[WARM:], KINDS[1]: b[:steps], KINDS[2]: b[steps:]}
    return out


def facade_drive(seed, range_noise):
    import parakeet_slam_amd as pk

    world, covs = synthetic_world(12, seed=5)
    start = world.copy()
    start[:, :2] += 0.5 * np.random.RandomState(100 + seed).standard_normal((12, 2))
    feats = [pk.Feature(mean=start[l].copy(), covar=covs[l].copy()) for l in range(12)]
    np.random.seed(seed)
    random.seed(seed)
    pk.msgs.Time.set_now(0.0)
    fs = pk.FastSLAM(feats, num_particles=64, device=0, weight_domain="log", rng="global", measurement_model="bearing", range_noise=range_noise)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = V, W
    fs.last_control = tw
    rs, rr = np.random.RandomState(seed), np.random.RandomState(1000 + seed)
    pose, err = (0.0, 0.0, 0.0), []

    class View(object):
        pass

    for s in range(40):
        pose = truth_step(pose, V, W, DT)
        blobs, rho, _ = scan_of(world, pose, rs, rr)
        view = View()
        view.last_sensor_reading = View()
        view.last_sensor_reading.observes = np.concatenate([blobs, rho[:, None]], axis=1) if range_noise else blobs
        pk.msgs.Time.set_now(DT * (s + 1))
        fs.cam_cb(view)
        x, y, _ = fs.summary()
        err.append(math.hypot(x - pose[0], y - pose[1]))
    means = fs._filter.download_landmarks()[0][:, :, :2].mean(axis=0)
    fs.close()
    return float(np.mean(np.hypot(*(means - world[:, :2]).T))), float(np.mean(err)), float(np.max(err))


if __name__ == "__main__":
    steps = int(arg("--steps", "10"))
    if "--trace" in sys.argv:
        trace_child(steps)
        sys.exit(0)
    out_path = arg("--out", os.path.join("out", "range_scan_cost.json"))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)

    t = kernel_trace(steps, os.path.join(os.path.dirname(out_path) or ".", "range_trace"))
    med = lambda v: sorted(v)[len(v) // 2]
    for stage, kinds in t.items():
        base = med(kinds[KINDS[0]])
        for kind in KINDS:
            v = kinds[kind]
            emit(dict(what="us per launch, from one kernel trace", particles=P, landmarks=L, blobs=L, kernel=stage, scan=kind, launches=len(v),
                      median=round(med(v), 2), min=round(min(v), 2), max=round(max(v), 2), ratio_to_no_range=round(med(v) / base, 3)))
    for seed in (1, 2, 3):
        for noise in (None, SIGMA_R):
            e, pm, px = facade_drive(seed, noise)
            emit(dict(what="pushed-map turning drive through the facade", seed=seed, range_noise=noise, landmark_error_m=round(e, 3),
                      pose_error_mean_m=round(pm, 3), pose_error_max_m=round(px, 3)))
    fh.close()

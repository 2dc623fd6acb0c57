"""What a step of a growing map costs with ranged scans (pk_grow_ranges; k_new_landmarks_tri_ranged, pk_k_grow.hip) against the
triangulated rule on bearings alone (k_new_landmarks_tri), on one GPU and one build: PK_T_OBSERVE per step -- the observe kernel
and the bookkeeping behind it, bracketed by events -- at 10 000 particles x (40 preset + 6 unknown landmarks, 8 spare slots) under
the bearing model, v 0.8, w 0.35, dt 0.5, 14 steps of noise-free wrapped scans, min_parallax 0.1, alternating, three runs each way
behind a warm-up of both.  One JSON line per run and one of medians.  A measurement, no threshold.
    python scripts/gpu_grow_ranges_cost.py [--out FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from oracle.fastslam_oracle import EMPTY_COLOUR, synthetic_world, truth_step  # noqa: E402
from parakeet_slam_amd import _lib  # noqa: E402

SIGMA = (0.05, 0.01)
V, W, DT = 0.8, 0.35, 0.5


def wrapped_scan(world, pose):
    x, y, h = pose
    blobs = np.empty((world.shape[0], 4))
    blobs[:, 0] = np.arctan2(world[:, 1] - y, world[:, 0] - x) - h
    blobs[:, 0] -= 2 * np.pi * np.rint(blobs[:, 0] / (2 * np.pi))
    blobs[:, 1:] = world[:, 2:]
    return blobs


def run(P, L0, U, spare, steps, ranged):
    world, covs = synthetic_world(L0 + U)
    means = np.zeros((L0 + spare, 5))
    means[:L0] = world[:L0]
    means[L0:, 2:] = EMPTY_COLOUR
    mcov = np.tile(np.identity(5).reshape(25), (L0 + spare, 1))
    mcov[:L0] = covs[:L0].reshape(L0, 25)
    f = _lib.DeviceFilter(P, L0 + spare, device=0)
    f.set_measurement_model("bearing")
    f.upload_map(means, mcov)
    f.grow_enable(L0, 64, 30.0)
    f.grow_init("triangulated", 0.1)
    if ranged:
        f.grow_ranges(True)
    f.enable_timing(True)
    pose, ms = (0.0, 0.0, 0.0), []
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose)
        f.reset_timings()
        f.motion(V, W, DT, seed=7, draw=s)
        if ranged:
            rho = np.hypot(world[:, 0] - pose[0], world[:, 1] - pose[1])
            f.scan_ranges(rho, (SIGMA[0] + SIGMA[1] * rho) ** 2)
        f.observe(blobs, fresh=True)
        f.resample(0.5, domain=_lib.PK_WEIGHTS_LOG)
        f.synchronize()
        ms.append(round(f.timings()["observe"][0], 4))
    cnt = f.grow_download(readings=False, slot_ids=False)[0]
    out = dict(observe_ms_per_step=ms, observe_ms_median=round(float(np.median(ms[1:])), 4), route=f.observe_route(),
               spare_slots_in_use_mean=round(float(cnt[:, 1].mean()), 3), readings_stored_mean=round(float(cnt[:, 0].mean()), 2))
    f.close()
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "grow_ranges_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    P, L0, U, spare, steps = 10000, 40, 6, 8, 14
    with open(out_path, "w") as fh:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        for ranged in (False, True):  # (the process's first launches, code objects loaded: not a figure)
            run(1024, L0, U, spare, 4, ranged)
        res = {False: [], True: []}
        for k in range(3):
            for ranged in (False, True):
                r = run(P, L0, U, spare, steps, ranged)
                res[ranged].append(r["observe_ms_median"])
                emit(dict(what="PK_T_OBSERVE per step", particles=P, preset=L0, unknown=U, spare=spare, ranged=ranged, run=k, **r))
        emit(dict(what="PK_T_OBSERVE per step, medians of the runs' medians (the first step left out)", particles=P,
                  triangulated=round(float(np.median(res[False])), 4), single_sighting=round(float(np.median(res[True])), 4)))


if __name__ == "__main__":
    main()

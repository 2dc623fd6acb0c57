"""What the measurement-informed proposal costs on a growing map (pk_proposal_grow) against the plain growing step, on one GPU and
one build: ms per step on the host clock -- pk_motion + pk_observe_fresh + pk_resample against pk_propose + pk_resample, each
behind a synchronisation -- at 10 000 particles x (40 preset + 6 unknown landmarks, 8 spare slots) under the bearing model, the
triangulated rule at 0.1 rad, v 0.8, w 0.35, dt 0.5, 14 steps of noise-free wrapped scans, on bearings alone and with a range on
every blob (pk_grow_ranges, pk_proposal_ranges), a fresh filter per run, the four variants alternating, three runs each behind a
warm-up of all.  One JSON line per run and one of medians.  A measurement, no threshold.
    python scripts/gpu_proposal_grow_cost.py [--out FILE]"""
import json
import os
import sys
import time

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


def run(P, L0, U, spare, steps, proposal, ranged):
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
    if proposal:
        f.proposal_grow(True)
        f.proposal_ranges(ranged)
    pose, ms = (0.0, 0.0, 0.0), []
    for s in range(steps):
        pose = truth_step(pose, V, W, DT)
        blobs = wrapped_scan(world, pose)
        rho = np.hypot(world[:, 0] - pose[0], world[:, 1] - pose[1])
        var = (SIGMA[0] + SIGMA[1] * rho) ** 2
        f.synchronize()
        t0 = time.perf_counter()
        if ranged:
            f.scan_ranges(rho, var)
        if proposal:
            f.propose(V, W, DT, blobs, seed=7, draw=s, fresh=True)
        else:
            f.motion(V, W, DT, seed=7, draw=s)
            f.observe(blobs, fresh=True)
        f.resample(0.5, domain=_lib.PK_WEIGHTS_LOG)
        f.synchronize()
        ms.append(round(1e3 * (time.perf_counter() - t0), 4))
    cnt = f.grow_download(readings=False, slot_ids=False)[0]
    out = dict(ms_per_step=ms, ms_median=round(float(np.median(ms[1:])), 4), route=f.observe_route(),
               spare_slots_in_use_mean=round(float(cnt[:, 1].mean()), 3), readings_stored_mean=round(float(cnt[:, 0].mean()), 2))
    f.close()
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "proposal_grow_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    P, L0, U, spare, steps = 10000, 40, 6, 8, 14
    variants = [(False, False), (True, False), (False, True), (True, True)]  # (proposal, ranged)
    with open(out_path, "w") as fh:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        for proposal, ranged in variants:  # (the process's first launches, code objects loaded: not a figure)
            run(1024, L0, U, spare, 4, proposal, ranged)
        res = {v: [] for v in variants}
        for k in range(3):
            for proposal, ranged in variants:
                r = run(P, L0, U, spare, steps, proposal, ranged)
                res[(proposal, ranged)].append(r["ms_median"])
                emit(dict(what="ms per step", particles=P, preset=L0, unknown=U, spare=spare, proposal=proposal, ranged=ranged, run=k, **r))
        med = {v: round(float(np.median(res[v])), 4) for v in variants}
        emit(dict(what="ms per step, medians of the runs' medians (the first step left out)", particles=P,
                  plain_bearings=med[(False, False)], proposal_bearings=med[(True, False)],
                  plain_ranged=med[(False, True)], proposal_ranged=med[(True, True)],
                  ratio_bearings=round(med[(True, False)] / med[(False, False)], 3),
                  ratio_ranged=round(med[(True, True)] / med[(False, True)], 3)))


if __name__ == "__main__":
    main()

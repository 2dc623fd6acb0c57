"""What retiring stale readings and unconfirmed features costs and buys (pk_grow_retire; pk_k_grow_retire.hip) on one GPU.  One
call, one JSON line per figure:
  1. on against off at 10 000 particles x (40 preset + 6 unknown) landmarks, bench.py's refscene.new_landmarks scene (12 steps,
     A = 4, M = 3): ms per step of cam_cb + summary() while the maps grow and afterwards, alternating, three runs each way;
  2. at scale, on against off: 20 000 x 2 000 + 16 spare slots (the scene of scripts/gpu_diag_grow_scale.py), 20 steps: per step
     the share of the particles the one-pass kernel handed to the fall-back kernels, the spare slots in use and ms per step.
--trace on|off: nothing but the steps of figure 1 (--steps N, default 12; --scale: of figure 2) on a fresh filter, for `rocprofv3 --kernel-trace --stats`
(a run of its own, no counters): k_grow_retire's time beside k_new_landmarks', or -- off, four steps, with --lib NAME another build
of the library, one from before these entry points existed too -- the kernels and counts of a step that retires nothing.
    python scripts/gpu_grow_retire_cost.py [--out FILE]"""
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the scenes' inputs)
import parakeet_slam_amd as pk  # noqa: E402
from parakeet_slam_amd import _lib  # noqa: E402

RETIRE_SYMBOLS = ("pk_grow_retire", "pk_grow_clocks_download", "pk_grow_clocks_upload")
A, M = 4, 3


class Scan(object):
    pass


class Node(object):
    pass


def growing_run(P, L0, U, spare, steps, retire, look=True):
    """bench.py's facade_growing with the thresholds as an argument; look: the counters after every step (outside the timed part)."""
    means, covs, _ = bench.synthetic_inputs(L0 + U, 1)
    feats = [pk.Feature(mean=means[l], covar=covs[l]) for l in range(L0)]
    pk.msgs.Time.set_now(0.0)
    random.seed(7)
    kw = dict(reading_max_age=A, potential_max_idle=M) if retire else {}
    fs = pk.FastSLAM(feats, num_particles=P, device=0, weight_domain="log", rng="device", seed=7, new_landmarks=True, spare_landmarks=spare,
                     publish_debug=False, **kw)
    node = Node()
    node.last_sensor_reading = Scan()
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = 0.5, 0.2
    fs.last_control = tw
    pose, dts, used, stored, flagged = (0.0, 0.0, 0.0), [], [], [], []
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
        dts.append((time.perf_counter() - t0) * 1e3)
        if look:
            c = fs._filter.grow_download(readings=False, slot_ids=False)[0]
            used.append(round(float(c[:, 1].mean()), 3))
            stored.append(round(float(c[:, 0].mean()), 2))
            flagged.append(int(fs._filter.observe_flagged()[0]))
    out = dict(ms_per_step=[round(x, 3) for x in dts], spare_slots_in_use_mean=used, readings_stored_mean=stored, flagged=flagged,
               route=fs._filter.observe_route(), readings_dropped=fs.readings_dropped() if look else None, retired=fs.retired() if look else None)
    if look:
        k = fs._filter.download_landmarks(means=False, covs=False)[2][:, L0:]
        u = fs._filter.grow_download(readings=False, slot_ids=False)[0][:, 1]
        out["promoted_per_particle"] = round(float((((k & 0x40000000) == 0) & (np.arange(k.shape[1])[None, :] < u[:, None])).sum() / float(P)), 3)
    fs.close()
    return out


def small(emit, P=10000, L0=40, U=6, steps=12, runs=3):
    growing_run(1024, L0, U, U + 2, 4, True)  # (the process's first launches, code objects loaded: not a figure)
    res = {False: [], True: []}
    for run in range(runs):
        for retire in (False, True):
            r = growing_run(P, L0, U, U + 2, steps, retire)
            used = r["spare_slots_in_use_mean"]
            growing = [i for i in range(1, steps) if used[i] > used[i - 1]]
            last = max(growing) if growing else 0
            r["ms_per_step_while_maps_grow"] = round(float(np.mean([r["ms_per_step"][i] for i in growing])), 3) if growing else None
            r["ms_per_step_afterwards"] = round(float(np.mean(r["ms_per_step"][last + 1:])), 3) if last + 1 < steps else None
            res[retire].append(r)
            emit(dict(what="on against off", particles=P, preset=L0, unknown=U, spare=U + 2, steps=steps, retirement=retire,
                      reading_max_age=A if retire else 0, potential_max_idle=M if retire else 0, run=run, **r))
    med = lambda rs, key: round(float(np.median([r[key] for r in rs if r[key] is not None])), 3)  # noqa: E731
    emit(dict(what="on against off, medians of the runs", particles=P, preset=L0, unknown=U, runs=runs,
              off_ms_while_maps_grow=med(res[False], "ms_per_step_while_maps_grow"), on_ms_while_maps_grow=med(res[True], "ms_per_step_while_maps_grow"),
              off_ms_afterwards=med(res[False], "ms_per_step_afterwards"), on_ms_afterwards=med(res[True], "ms_per_step_afterwards")))


def at_scale(emit, P=20000, L0=2000, U=6, spare=16, steps=20):
    for retire in (False, True):
        r = growing_run(P, L0, U, spare, steps, retire)
        r["share_on_the_fall_back_kernels"] = [round(x / float(P), 4) for x in r.pop("flagged")]
        emit(dict(what="at scale", particles=P, preset=L0, unknown=U, spare=spare, steps=steps, retirement=retire,
                  reading_max_age=A if retire else 0, potential_max_idle=M if retire else 0, **r))


if __name__ == "__main__":
    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.join(ROOT, "parakeet_slam_amd", sys.argv[sys.argv.index("--lib") + 1])
        import ctypes

        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in RETIRE_SYMBOLS:  # a build from before these entry points: bind what it has
            if not hasattr(probe, name):
                _lib.SIGNATURES.pop(name, None)
    if "--trace" in sys.argv:
        on = sys.argv[sys.argv.index("--trace") + 1] == "on"
        steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 12
        shape = (20000, 2000, 6, 16) if "--scale" in sys.argv else (10000, 40, 6, 8)  # figure 2's scene, or figure 1's
        r = growing_run(*shape, steps, on, look=False)
        print(json.dumps(dict(what="trace", shape=shape, retirement=on, steps=steps, ms_per_step=r["ms_per_step"], route=r["route"])), flush=True)
        sys.exit(0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "grow_retire_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)
        return ln

    small(emit)
    at_scale(emit)
    fh.close()

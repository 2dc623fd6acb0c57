"""What the triangulated initialisation of growing maps costs and buys (pk_grow_init; k_new_landmarks_tri, pk_k_grow.hip) on one
GPU.  One call, one JSON line per figure:
  1. the rule off against on at 10 000 particles x (40 preset + 6 unknown) landmarks, bench.py's refscene.new_landmarks scene
     (12 steps, min_parallax 0.2): ms per step of cam_cb + summary() while the maps grow and afterwards, alternating, three runs
     each way, and their medians;
  2. the error table of DESIGN.md section 9 on the device, through the facade: the bearing model, 64 particles,
     synthetic_world(12, seed=5) with its last three landmarks unknown, 6 spare slots, pair threshold 30; v = 1.0, w = 0.35,
     dt = 0.5, bearings with sigma 0.01 rad and colours with 0.3 per channel, 60 steps, seeds 1-3: the distance of every spare
     feature in use, in every particle, from the unknown landmark of the nearest colour -- today's rule, any crossing with the
     propagated covariance (min_parallax 0), and min_parallax 0.2 with the propagated covariance.
--trace reference|triangulated: nothing but the steps of figure 1 (--steps N, default 12) on a fresh filter, for
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters): the time per launch of the bookkeeping kernel's instance.
    python scripts/gpu_grow_init_cost.py [--out FILE]"""
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the scene's inputs)
import parakeet_slam_amd as pk  # noqa: E402
from oracle.fastslam_oracle import synthetic_world, truth_step  # noqa: E402

MIN_PARALLAX = 0.2


class Scan(object):
    pass


class Node(object):
    pass


def growing_run(P, L0, U, spare, steps, rule, min_parallax=MIN_PARALLAX, look=True):
    """bench.py's facade_growing with the rule as an argument; look: the counters after every step (outside the timed part)."""
    means, covs, _ = bench.synthetic_inputs(L0 + U, 1)
    feats = [pk.Feature(mean=means[l], covar=covs[l]) for l in range(L0)]
    pk.msgs.Time.set_now(0.0)
    random.seed(7)
    fs = pk.FastSLAM(feats, num_particles=P, device=0, weight_domain="log", rng="device", seed=7, new_landmarks=True, spare_landmarks=spare,
                     publish_debug=False, landmark_init=rule, min_parallax=min_parallax)
    node = Node()
    node.last_sensor_reading = Scan()
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = 0.5, 0.2
    fs.last_control = tw
    pose, dts, used, stored = (0.0, 0.0, 0.0), [], [], []
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
    out = dict(ms_per_step=[round(x, 3) for x in dts], spare_slots_in_use_mean=used, readings_stored_mean=stored,
               route=fs._filter.observe_route(), readings_dropped=fs.readings_dropped() if look else None)
    fs.close()
    return out


def small(emit, P=10000, L0=40, U=6, steps=12, runs=3):
    growing_run(1024, L0, U, U + 2, 4, "triangulated")  # (the process's first launches, code objects loaded: not a figure)
    growing_run(1024, L0, U, U + 2, 4, "reference")
    res = {"reference": [], "triangulated": []}
    for run in range(runs):
        for rule in ("reference", "triangulated"):
            r = growing_run(P, L0, U, U + 2, steps, rule)
            r["ms_per_step_all"] = round(float(np.mean(r["ms_per_step"][1:])), 3)
            res[rule].append(r)
            emit(dict(what="off against on", particles=P, preset=L0, unknown=U, spare=U + 2, steps=steps, landmark_init=rule,
                      min_parallax=MIN_PARALLAX if rule == "triangulated" else None, run=run, **r))
    med = lambda rs, key: round(float(np.median([r[key] for r in rs])), 3)  # noqa: E731
    emit(dict(what="off against on, medians of the runs (ms per step, the first step left out)", particles=P, preset=L0, unknown=U, runs=runs,
              reference=med(res["reference"], "ms_per_step_all"), triangulated=med(res["triangulated"], "ms_per_step_all")))


def wrapped_scan(world, pose, rs, sigma_bearing, sigma_colour):
    x, y, h = pose
    B = world.shape[0]
    blobs = np.empty((B, 4))
    blobs[:, 0] = np.arctan2(world[:, 1] - y, world[:, 0] - x) - h + sigma_bearing * rs.standard_normal(B)
    blobs[:, 1:] = world[:, 2:] + sigma_colour * rs.standard_normal((B, 3))
    blobs[:, 0] -= 2 * math.pi * np.rint(blobs[:, 0] / (2 * math.pi))
    return blobs


def error_table(emit, P=64, L0=9, spare=6, steps=60):
    world, covs = synthetic_world(12, seed=5)
    feats = [pk.Feature(mean=world[l].copy(), covar=covs[l].copy()) for l in range(L0)]
    v, w, dt = 1.0, 0.35, 0.5
    for seed in (1, 2, 3):
        for name, kw in (("any crossing, identity covariance", dict()),
                         ("any crossing, propagated covariance", dict(landmark_init="triangulated", min_parallax=0.0)),
                         ("minimum parallax 0.2 rad, propagated covariance", dict(landmark_init="triangulated", min_parallax=0.2))):
            np.random.seed(seed)
            random.seed(seed)
            noise = np.random.RandomState(seed)
            pk.msgs.Time.set_now(0.0)
            fs = pk.FastSLAM(feats, num_particles=P, device=0, weight_domain="log", rng="global", new_landmarks=True, spare_landmarks=spare,
                             pair_threshold=30.0, measurement_model="bearing", publish_debug=False, **kw)
            tw = pk.msgs.Twist()
            tw.linear.x, tw.angular.z = v, w
            fs.last_control = tw
            node = Node()
            node.last_sensor_reading = Scan()
            pose = (0.0, 0.0, 0.0)
            for s_ in range(steps):
                pose = truth_step(pose, v, w, dt)
                pk.msgs.Time.set_now(dt * (s_ + 1))
                node.last_sensor_reading.observes = wrapped_scan(world, pose, noise, 0.01, 0.3)
                fs.cam_cb(node)
            m = fs._filter.download_landmarks(covs=False, counts=False)[0]
            used = fs._filter.grow_download(readings=False, slot_ids=False)[0][:, 1]
            e = []
            for i in range(P):
                for k in range(int(used[i])):
                    f = m[i, L0 + k]
                    j = int(np.argmin(np.linalg.norm(world[L0:, 2:] - f[2:], axis=1)))
                    e.append(float(np.hypot(f[0] - world[L0 + j, 0], f[1] - world[L0 + j, 1])))
            s = fs.summary()
            emit(dict(what="error table on the device", initialisation=name, seed=seed, particles=P, steps=steps,
                      median_m=round(float(np.median(e)), 3), mean_m=round(float(np.mean(e)), 3), max_m=round(float(np.max(e)), 2),
                      spare_slots_in_use=sorted(set(int(u) for u in used)), readings_dropped=fs.readings_dropped(),
                      pose_error_m=round(float(math.hypot(s[0] - pose[0], s[1] - pose[1])), 3)))
            fs.close()


if __name__ == "__main__":
    if "--trace" in sys.argv:
        rule = sys.argv[sys.argv.index("--trace") + 1]
        steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 12
        r = growing_run(10000, 40, 6, 8, steps, rule, look=False)
        print(json.dumps(dict(what="trace", landmark_init=rule, steps=steps, ms_per_step=r["ms_per_step"], route=r["route"])), flush=True)
        sys.exit(0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("out", "grow_init_cost.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)
        return ln

    small(emit)
    error_table(emit)
    fh.close()

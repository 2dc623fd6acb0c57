"""What the field of view costs the retirement pass (pk_grow_view; DESIGN.md section 9, "A field of view for retirement"): the
PK_T_OBSERVE time of pk_timings -- the observe kernels, the new-landmark bookkeeping and the retirement pass behind it -- per step on
the growing scene of scripts/gpu_grow_speed.py, retirement on (A = 4, M = 3), without a view and with one (+-1 rad, 0.5 to 25 m,
C = 4), runs alternating.  Prints one JSON line.
    python scripts/gpu_grow_view_cost.py [P] [L0] [U] [steps] [runs]"""
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import parakeet_slam_amd as pk  # noqa: E402
from gpu_grow_speed import View, ring_world, scan  # noqa: E402

VIEW, C = (1.0, 0.5, 25.0), 4


def run(P, L0, U, steps, view):
    world = ring_world(L0 + U)
    feats = [pk.Feature(mean=world[l].copy(), covar=0.25 * np.identity(5)) for l in range(L0)]
    random.seed(3)
    pk.msgs.Time.set_now(0.0)
    kw = dict(view=VIEW, confirmed_max_misses=C) if view else {}
    fs = pk.FastSLAM(feats, num_particles=P, weight_domain="log", rng="device", seed=3, new_landmarks=True, spare_landmarks=U + 2,
                     publish_debug=False, reading_max_age=4, potential_max_idle=3, **kw)
    tw = pk.msgs.Twist()
    tw.linear.x, tw.angular.z = 0.5, 0.2
    fs.last_control = tw
    f = fs._filter
    f.enable_timing(True)
    pose, t = (0.0, 0.0, 0.0), []
    for s in range(steps):
        h1 = pose[2] + 0.2 * 0.1
        pose = (pose[0] + 0.1 * np.cos(h1), pose[1] + 0.1 * np.sin(h1), pose[2] + 0.04)
        pk.msgs.Time.set_now(0.2 * (s + 1))
        f.reset_timings()
        fs.cam_cb(View(scan(world, pose)))
        fs.summary()
        t.append(f.timings()["observe"][0])
    out = dict(observe_ms_per_step=[round(x, 4) for x in t], median_ms=round(float(np.median(t[1:])), 4), retired=fs.retired())
    if view:
        out["view_stats"] = fs.view_stats()
    fs.close()
    return out


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    P, L0, U, steps, runs = (a + [10000, 40, 6, 12, 3][len(a):])[:5]
    res = dict(particles=P, preset_landmarks=L0, unknown_landmarks=U, steps=steps, view=VIEW, confirmed_max_misses=C, without_view=[], with_view=[])
    for _ in range(runs):
        res["without_view"].append(run(P, L0, U, steps, False))
        res["with_view"].append(run(P, L0, U, steps, True))
    for k in ("without_view", "with_view"):
        res[k + "_median_ms"] = round(float(np.median([r["median_ms"] for r in res[k]])), 4)
    print(json.dumps(res))

"""What the bearing measurement model costs (pk_set_measurement_model(f, PK_MODEL_BEARING); DESIGN.md section 4, "The bearing model") on
one GPU, on the benchmark's own world and scans (bench.synthetic_inputs: headings within +-0.6 rad, where both models match the same
blobs) at the shapes of BASELINE.json configs[1] (10 000 x 500) and configs[2] (100 000 x 2 000).  Three variants, a fresh filter per
run, alternating in one call, three runs each:
  bearing            the bearing model: k_assoc_grid_bearing + k_observe_bearing (PK_ROUTE_ML_GENERAL)
  reference_general  the reference model forced onto the same general route (option "fast_observe" = 0, as the route tests force it):
                     k_assoc_grid<GENERAL> + k_observe -- the model's own cost is bearing against this
  reference_default  the reference model on the route it takes by itself (one-pass): the gap the follow-up has to win back
Per run: WARM untimed steps, then STEPS pk_step (device noise, log-domain resample) between two synchronisations on the host clock
-> ms per step; then the same steps of the same drive on another fresh filter with pk_enable_timing on (hipEvents around the
PK_T_ASSOC and PK_T_OBSERVE launches: on the general route the first holds the association kernel alone, the second k_observe
alone) -> ms per launch of each.
One JSON line per run and one summary line per shape.
    python scripts/gpu_bearing_model_cost.py [--out FILE] [--steps N] [--shapes PxL,PxL]"""
import json
import os
import random
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from parakeet_slam_amd import _lib  # noqa: E402

LOG = _lib.PK_WEIGHTS_LOG
WARM = 3
VARIANTS = (("bearing", "bearing", {}), ("reference_general", "reference", {"fast_observe": 0}), ("reference_default", "reference", {}))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def drive(P, L, model, opts, means, covs, scans, ws, steps, timed):
    """WARM + steps steps on a fresh filter; the steps behind the warm-up on the host clock, or (timed) under pk_enable_timing."""
    f = _lib.DeviceFilter(P, L)
    f.set_measurement_model(model)
    for k, v in opts.items():
        f.set_option(k, v)
    f.upload_map(means, covs.reshape(L, 25))
    rnd = random.Random(7)
    s = 0

    def run(n):
        nonlocal s
        for _ in range(n):
            f.step(0.2, ws[s], 0.1, scans[s], rnd.random(), seed=7, draw=s, domain=LOG)
            s += 1
        f.synchronize()

    run(WARM)
    if timed:
        f.enable_timing(-1)
        f.reset_timings()
    t0 = time.perf_counter()
    run(steps)
    ms_step = (time.perf_counter() - t0) * 1e3 / steps
    out = (ms_step, f.observe_route(), f.timings() if timed else None, f.summary())
    f.close()
    return out


def one_run(P, L, model, opts, means, covs, scans, ws, steps):
    ms_step, route, _, summary = drive(P, L, model, opts, means, covs, scans, ws, steps, False)
    _, _, t, again = drive(P, L, model, opts, means, covs, scans, ws, steps, True)  # the SAME steps, bracketed by events
    assert again == summary, (again, summary)
    per = {k: (round(t[k][0] / t[k][1], 5) if t[k][1] else None) for k in ("assoc", "observe")}
    return dict(route=route, ms_per_step=round(ms_step, 4), assoc_ms_per_launch=per["assoc"], observe_ms_per_launch=per["observe"],
                assoc_launches_per_step=t["assoc"][1] / steps, observe_launches_per_step=t["observe"][1] / steps,
                assoc_ms_per_step=round(t["assoc"][0] / steps, 4), observe_ms_per_step=round(t["observe"][0] / steps, 4), summary=summary)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


if __name__ == "__main__":
    out_path = arg("--out", os.path.join("out", "bearing_model_cost.json"))
    steps = int(arg("--steps", "20"))
    shapes = [tuple(int(x) for x in sh.split("x")) for sh in arg("--shapes", "10000x500,100000x2000").split(",")]
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    fh = open(out_path, "w")

    def emit(ln):
        fh.write(json.dumps(ln) + "\n")
        fh.flush()
        print(json.dumps(ln), flush=True)

    for P, L in shapes:
        means, covs, scans = bench.synthetic_inputs(L, WARM + steps)
        ws = bench.synthetic_controls(WARM + steps)
        runs = {name: [] for name, _, _ in VARIANTS}
        for repeat in (1, 2, 3):
            for name, model, opts in VARIANTS:  # alternating
                r = one_run(P, L, model, opts, means, covs, scans, ws, steps)
                runs[name].append(r)
                emit(dict(what="run", particles=P, landmarks=L, blobs=L, variant=name, repeat=repeat, steps=steps, **r))
        med = {name: {k: median([r[k] for r in rs]) for k in ("ms_per_step", "assoc_ms_per_step", "observe_ms_per_step")} for name, rs in runs.items()}
        spread = {name: round((max(r["ms_per_step"] for r in rs) - min(r["ms_per_step"] for r in rs)) / med[name]["ms_per_step"], 4)
                  for name, rs in runs.items()}
        b, g, d = med["bearing"], med["reference_general"], med["reference_default"]
        emit(dict(what="medians of three", particles=P, landmarks=L, medians=med, spread_of_ms_per_step=spread,
                  bearing_over_reference_general=dict(step=round(b["ms_per_step"] / g["ms_per_step"], 4),
                                                      assoc=round(b["assoc_ms_per_step"] / g["assoc_ms_per_step"], 4),
                                                      observe=round(b["observe_ms_per_step"] / g["observe_ms_per_step"], 4)),
                  bearing_over_reference_default_step=round(b["ms_per_step"] / d["ms_per_step"], 4)))
    fh.close()

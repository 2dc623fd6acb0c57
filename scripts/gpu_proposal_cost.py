"""What the measurement-informed proposal costs (pk_propose; DESIGN.md section 4, "The measurement-informed proposal") on one GPU, on
the benchmark's own world and scans (bench.synthetic_inputs) at the shapes of BASELINE.json configs[1] (10 000 x 500) and configs[2]
(100 000 x 2 000).  Two variants on bearing-model filters, a fresh filter per run, alternating in one call, three runs each:
  bearing   the plain step: pk_motion + pk_observe_fresh (k_assoc_grid_bearing + k_observe_bearing, PK_ROUTE_ML_GENERAL) + pk_resample
  proposal  pk_propose(fresh) + pk_resample: the motion kernel twice, the same association, k_propose, k_observe_proposed
Per run: WARM untimed steps, then STEPS steps (device noise, log-domain resample) between two synchronisations on the host clock ->
ms per step; then the same steps of the same drive on another fresh filter with pk_enable_timing on (hipEvents around the launches of
every PK_T_* span: assoc holds the association kernel alone, propose k_propose alone, observe the EKF kernel alone) -> ms per step of
each, and n_eff / P of the weights in front of every resample (which synchronises: that pass is not the one on the host clock).
One JSON line per run and one summary line per shape.
    python scripts/gpu_proposal_cost.py [--out FILE] [--steps N] [--shapes PxL,PxL]"""
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
VARIANTS = ("bearing", "proposal")
SPANS = ("motion", "assoc", "propose", "observe", "resample")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def drive(P, L, variant, means, covs, scans, ws, steps, timed):
    f = _lib.DeviceFilter(P, L)
    f.set_measurement_model("bearing")
    f.upload_map(means, covs.reshape(L, 25))
    rnd = random.Random(7)
    s = 0
    neff = []

    def run(n, measure):
        nonlocal s
        for _ in range(n):
            if variant == "proposal":
                f.propose(0.2, ws[s], 0.1, scans[s], seed=7, draw=s, fresh=True)
            else:
                f.motion(0.2, ws[s], 0.1, seed=7, draw=s)
                f.observe(scans[s], fresh=True)
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


def one_run(P, L, variant, means, covs, scans, ws, steps):
    ms_step, route, _, summary, _ = drive(P, L, variant, means, covs, scans, ws, steps, False)
    _, _, t, again, neff = drive(P, L, variant, means, covs, scans, ws, steps, True)  # the SAME steps, bracketed by events
    assert again == summary, (again, summary)
    out = dict(route=route, ms_per_step=round(ms_step, 4), n_eff_over_P=round(sum(neff) / len(neff), 4), summary=summary)
    for k in SPANS:
        out[k + "_ms_per_step"] = round(t[k][0] / steps, 4)
        out[k + "_launches_per_step"] = t[k][1] / steps
    return out


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


if __name__ == "__main__":
    out_path = arg("--out", os.path.join("out", "proposal_cost.json"))
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
        runs = {name: [] for name in VARIANTS}
        for repeat in (1, 2, 3):
            for name in VARIANTS:  # alternating
                r = one_run(P, L, name, means, covs, scans, ws, steps)
                runs[name].append(r)
                emit(dict(what="run", particles=P, landmarks=L, blobs=L, variant=name, repeat=repeat, steps=steps, **r))
        keys = ["ms_per_step", "n_eff_over_P"] + [k + "_ms_per_step" for k in SPANS]
        med = {name: {k: median([r[k] for r in rs]) for k in keys} for name, rs in runs.items()}
        spread = {name: round((max(r["ms_per_step"] for r in rs) - min(r["ms_per_step"] for r in rs)) / med[name]["ms_per_step"], 4)
                  for name, rs in runs.items()}
        b, p = med["bearing"], med["proposal"]
        emit(dict(what="medians of three", particles=P, landmarks=L, medians=med, spread_of_ms_per_step=spread,
                  proposal_over_bearing_step=round(p["ms_per_step"] / b["ms_per_step"], 4),
                  k_propose_over_association=round(p["propose_ms_per_step"] / p["assoc_ms_per_step"], 4),
                  k_propose_over_observe=round(p["propose_ms_per_step"] / p["observe_ms_per_step"], 4)))
    fh.close()

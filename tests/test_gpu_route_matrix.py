"""GPU: which kernels a scan gets (pk_api_observe.hip: plan_scan; DESIGN.md section 4, "Routing").  One filter per row of a matrix of map
sizes (each beside a routing boundary), scan sizes and settings; two scans with a resample between them; after each scan the route,
the publish table's figures, the flagged particles, the second-chance rows, the colour table's statistics and the launches per
timing slot are compared, exactly, with tests/golden/route_matrix.json.

The fixture holds what the library did BEFORE the routing moved into one plan; it is recorded with

    python tests/test_gpu_route_matrix.py --record [--lib path/to/libparakeet_slam.so]

from a build of the commit whose routing is to be preserved, never from the code under test."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script: --record)
    sys.path.insert(0, ROOT)

from oracle.fastslam_oracle import EMPTY_COLOUR, synthetic_world  # noqa: E402
from test_gpu_colour_table import scan_of, truth  # noqa: E402
from test_gpu_pub import poses_around  # noqa: E402

pytestmark = pytest.mark.gpu

P = 64
LOG = 1  # PK_WEIGHTS_LOG
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_matrix.json")
SIZES = (40, 300, 512, 513, 1030, 2048, 2049, 3000, 6144, 6145)  # L <= 512 | <= 2 048 | <= 6 144 | beyond


def _rows():
    rows = []

    def row(L, B, opts=None, mode="observe"):
        name = "L%d-B%d-%s" % (L, B, mode) + "".join("-%s=%d" % kv for kv in sorted((opts or {}).items()))
        rows.append(dict(name=name, L=L, B=B, opts=opts or {}, mode=mode))

    for L in SIZES:
        row(L, 40)
        row(L, 8)
    for L in (40, 1030, 3000):
        row(L, 0)
    for L in (300, 512):
        row(L, 40, {"fused_step": 0})
    for L in (1030, 2048):
        row(L, 40, {"regs_step": 0})
    for L in (1030, 3000):
        row(L, 40, {"pub_step": 0})
        row(L, 40, {"cand_lists": 0})
        row(L, 40, {"far_prune": 0})
        row(L, 40, {"pub_entry_limit": 1})
        row(L, 40, {"fast_observe": 2})
    row(300, 40, {"pub_small": 0})
    for L in (40, 300, 512, 513):
        row(L, 40, {"pub_small": 1})
    row(300, 40, {"pub_small": 1, "cand_lists": 0})
    row(300, 40, {"pub_small": 1, "far_prune": 0})
    row(300, 40, {"pub_small": 1, "pub_entry_limit": 1})
    row(1030, 40, {"far_prune": 0, "pub_entry_limit": 1})
    for L in (300, 1030):
        row(L, 40, {"fast_observe": 0})
        row(L, 40, {"assoc_kernel": 1})
        row(L, 40, mode="supplied_ids")
    row(300, 40, {"fast_observe": 2})
    for L in (300, 3000):
        row(L, 40, {"fast_observe": 3})
    for L in (300, 1030, 3000):
        row(L, 40, {"assoc_dup": 0})
        row(L, 40, mode="ids_out")
        row(L, 40, mode="grow")
        row(L, 40, mode="step")
        row(L, 40, mode="staged")
    row(1030, 8, mode="grow")
    row(1030, 40, {"pub_step": 0}, mode="grow")
    for duo in (1, 2):
        row(3000, 40, {"pub_duo": duo})
    row(1030, 40, {"regs_retry": 0})
    row(1030, 40, {"regs_retry": 0, "pub_step": 0})
    for L in (513, 1030):
        row(L, 40, {"colour_table": 0})
    row(300, 0, mode="step")
    row(6145, 40, mode="step")
    row(6145, 40, mode="staged")
    for L in (1030, 3000):
        row(L, 40, mode="staged_range")
    return rows


ROWS = _rows()


def run_row(lib, r, on_done=None):
    """The row's two scans; what the library says about each.  on_done(filter): called before the filter is closed."""
    L, B, mode = r["L"], r["B"], r["mode"]
    rs = np.random.RandomState(1000 + L + B)
    means, covs = synthetic_world(L)
    known = L - 4 if mode == "grow" else L  # growing maps: four spare slots behind the known landmarks
    if mode == "grow":
        means[known:, :2] = 0.0
        means[known:, 2:] = EMPTY_COLOUR
    seen = np.linspace(0, known - 1, B).astype(int) if B else np.zeros(0, dtype=int)  # the blobs are sightings of map landmarks
    f = lib.DeviceFilter(P, L)
    for k, v in r["opts"].items():
        f.set_option(k, v)
    f.enable_timing(True)
    f.upload_map(means, covs.reshape(L, 25))
    f.upload_poses(poses_around(rs, P))
    if mode == "grow":
        f.grow_enable(known, 64, 30.0)
    path = truth(2)
    out = []
    for s in range(2):
        pose = path[s] if mode == "step" else (0.0, 0.0, 0.0)
        blobs = scan_of(means, pose, seen)
        rec = {}
        if mode == "step":
            f.step(0.2, 0.05, 0.1, blobs, 0.37, seed=5, draw=s, domain=LOG)
        elif mode == "supplied_ids":
            f.observe(blobs, ids=seen + 1)
        elif mode == "ids_out":
            f.observe(blobs, return_ids=True)
        elif mode in ("staged", "staged_range"):
            f.stage_scan(blobs)
            rec["takes_regs"] = int(f.staged_takes_regs())
            if mode == "staged":
                f.observe_staged()
            else:
                f.observe_staged_range(False, 0, 24, True, False)
                f.observe_staged_range(False, 24, P, False, True)
        else:
            f.observe(blobs)
        rec["route"] = f.observe_route()
        rec["published"] = int(f.observe_published())
        rec["pub_stats"] = list(f.observe_pub_stats().values())  # entries, contested, multi, longest list, capacity, instance
        rec["flagged"] = list(f.observe_flagged())
        rec["retry_capacity"] = f.observe_retry_rows()[1]
        rec["colour_table"] = list(f.colour_table_stats().values())  # engaged, depth, scans, materialisations
        rec["launches"] = {k: v[1] for k, v in f.timings().items() if v[1]}  # per slot, since the filter was made
        out.append(rec)
        if s == 0 and mode != "step":
            f.resample(0.37, domain=LOG)
    if on_done is not None:
        on_done(f)
    f.close()
    return out


def record(lib):
    return {r["name"]: run_row(lib, r) for r in ROWS}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_matrix_is_the_fixtures(golden):
    assert sorted(golden) == sorted(r["name"] for r in ROWS)


@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_every_scan_takes_the_kernels_it_took(lib, golden, r):
    assert run_row(lib, r) == golden[r["name"]]


if __name__ == "__main__":
    from parakeet_slam_amd import _lib

    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    got = record(_lib)
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as fh:
            fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(got[k], separators=(",", ":"), sort_keys=True)) for k in sorted(got)) + "\n}\n")
        print("recorded %d rows from %s" % (len(got), _lib.LIB_PATH))
    else:
        with open(FIXTURE) as fh:
            want = json.load(fh)
        bad = [k for k in want if got.get(k) != want[k]]
        print("%d rows, %d differ from the fixture: %s" % (len(got), len(bad), bad))
        sys.exit(1 if bad else 0)

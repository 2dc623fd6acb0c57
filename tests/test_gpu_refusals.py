"""GPU: what the C ABI refuses, and with which words (pk_api.hip: pk_set_option, pk_resample; pk_api_shard.hip: the shard, pack and
adopt entry points; the option table is in pk_filter.hpp).  A list of named bad calls on filters of 16 particles x 8 landmarks --
every option below, above and at both ends of its range, the entry points that refuse a growing filter, an active balanced
placement or a missing plan, calls to which two refusals apply at once (the order of the checks is part of the behaviour), NULL
handles -- each recorded as [status, message], or "ok" for the accepted neighbour of a boundary, and compared, exactly, with
tests/golden/refusals.json.

Every case ends in a refusal or a plain success.  Where an entry point wants a device buffer it gets a real one, large enough for
what the call would write if it were not refused; 0 is passed only where NULL itself is the bad argument.

The fixture holds what the library answered BEFORE the host layer was split into three files and the refusals were stated once; it
is recorded with

    python tests/test_gpu_refusals.py --record [--lib path/to/libparakeet_slam.so]

from a build of the commit whose answers are to be preserved, never from the code under test.

tests/golden/scan_refusals.json holds, in the same way, what the calls that take a scan -- pk_observe, pk_observe_fresh, pk_associate,
pk_stage_scan, pk_step, pk_propose and pk_propose_odom (the last two on bearing-model filters) -- answer to bad arguments
(record_scan): B < 0, blobs missing, no map, a NaN in blob 1 (the message names the blob, not the double), ids of -1 and L + 1 with
L accepted, supplied ids on a growing filter, B = 0, 65 536 blobs without ids, pk_associate without ids_out, and the pairs that show
each call's order of checks (no map + NaN, NaN + bad id, armed ranges of another length + NaN, the reference model + bad blobs for
pk_propose).  It was recorded by the same command from a build of the commit BEFORE these checks and the per-scan block's layout
were stated once (pk_api_scan.hip, pk_scan_block.hpp), on the GPU, never from the code under test; --record writes both fixtures."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script: --record)
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

P, L = 16, 8
LINEAR, LOG = 0, 1
FIXTURE = os.path.join(ROOT, "tests", "golden", "refusals.json")
SCAN_FIXTURE = os.path.join(ROOT, "tests", "golden", "scan_refusals.json")
SCRATCH_BYTES = 1 << 20

# option -> inclusive range (P: the number of particles), in the order pk_set_option is asked; None: any value is taken
OPTIONS = {
    "assoc_kernel": (0, 1), "assoc_dup": None, "fast_observe": (0, 3), "timing_stride": (1, 1000000), "upload_kernel": None,
    "fused_step": None, "cand_lists": None, "pub_step": None, "pub_small": None, "far_prune": None, "pub_duo": (0, 2),
    "pub_duo_park_limit": (-1, 65535), "pub_entry_limit": (0, 65534), "regs_step": None, "split_loopback_lo": (0, P),
    "split_loopback_hi": (0, P), "balanced_loopback_keep": (-1, P), "split_reserve_cus": (0, 128), "regs_retry": (0, 1),
    "regs_warm": (0, 2), "colour_table": (-1, 1), "colour_table_depth": (8, 32768), "colour_table_margin": (-1, 32768),
    "observe_landmarks_per_lane": (0, 2),  # (process-wide: its last case leaves it at 0, the default)
}


class Hip(object):
    """hipMalloc / hipMemcpy / hipFree of the runtime the library itself has loaded."""

    def __init__(self):
        with open("/proc/self/maps") as fh:
            paths = sorted({ln.split()[-1] for ln in fh if "libamdhip64" in ln})
        self.rt = C.CDLL(paths[0])
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.blocks = []

    def zeros(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), nbytes) == 0 and p.value
        assert self.rt.hipMemset(p, 0, nbytes) == 0
        self.blocks.append(p)
        return p.value

    def to_host(self, ptr, dtype, n):
        out = np.empty(n, dtype=dtype)
        assert self.rt.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free_all(self):
        for p in self.blocks:
            self.rt.hipFree(p)
        self.blocks = []


def record(lib):
    """Every case in order: name -> "ok" | [status, message]."""
    abi = lib.load()
    hip = Hip()
    buf = hip.zeros(SCRATCH_BYTES)      # records in and out
    state = hip.zeros(2 * P * 8)        # pk_shard_state_dev of one rank: log-weights | logical indices
    table_dev = hip.zeros(6 * 8)        # the balanced plan's table of a world of one
    out = {}

    def call(case, fn, *args):
        assert case not in out, case
        st = getattr(abi, fn)(*args)
        out[case] = "ok" if st == lib.PK_OK else [int(st), abi.pk_last_error().decode()]

    def new_filter():
        f = lib.DeviceFilter(P, L)
        means = np.column_stack([np.linspace(-4.0, 4.0, L), np.linspace(3.0, 5.0, L), np.linspace(10.0, 220.0, L), np.full(L, 50.0), np.full(L, 90.0)])
        f.upload_map(means, np.tile(0.25 * np.identity(5), (L, 1, 1)).reshape(L, 25))
        poses = np.zeros((P, 4))
        poses[:, 3] = 1.0
        f.upload_poses(poses)
        assert f.particle_bytes() * P <= SCRATCH_BYTES
        return f

    def host_plan(f):  # the host-side offspring plan of a world of one: pk_shard_max_logw / block_totals / offspring
        f.shard_offspring(f.shard_block_totals(f.shard_max_logw(), LOG), 0, P, 0.37, True)

    lp = lib.lptr
    iota = np.arange(P, dtype=np.int64)
    one = np.zeros(1, dtype=np.int64)
    ranges = np.zeros(2, dtype=np.int64)
    no_table = np.zeros(6, dtype=np.int64)
    hi = np.empty(P + 1, dtype=np.int64)
    rel, Hl, alive = np.empty(P + 1, dtype=np.int64), np.empty(P, dtype=np.int64), np.empty(P, dtype=np.int32)
    totals = np.ones(1)

    # ---- options
    f = new_filter()
    h = f._h
    for name, rng in OPTIONS.items():
        values = (-5, 7, 1, 0) if rng is None else (rng[0] - 1, rng[1] + 1, rng[1], rng[0])
        for v in values:
            call("option-%s=%d" % (name, v), "pk_set_option", h, name.encode(), v)
    call("option-unknown", "pk_set_option", h, b"no_such_option", 1)
    call("option-empty-name", "pk_set_option", h, b"", 1)
    call("option-prefix-of-a-name", "pk_set_option", h, b"pub_duo_park", 1)
    call("option-null-name", "pk_set_option", h, None, 1)
    call("option-null-handle", "pk_set_option", None, b"pub_step", 1)
    f.close()

    # ---- a plain filter: no plan yet, then argument checks, then a plan
    f = new_filter()
    h = f._h
    call("noplan-shard_download_offspring", "pk_shard_download_offspring", h, lp(hi))
    call("noplan-shard_pack_dev", "pk_shard_pack_dev", h, lp(ranges), 1, 0, buf)
    call("noplan-shard_pack_slots_dev", "pk_shard_pack_slots_dev", h, 0, 0, 0, 0, buf)
    call("noplan-shard_adopt_dev", "pk_shard_adopt_dev", h, 0, buf, 0)
    call("noplan-shard_adopt_local_dev", "pk_shard_adopt_local_dev", h, 0)
    call("noplan-shard_adopt_remote_dev", "pk_shard_adopt_remote_dev", h, 0, buf, 0)
    call("noplan-shard_local_span_dev", "pk_shard_local_span_dev", h, buf)
    call("noplan-shard_download_balanced_plan", "pk_shard_download_balanced_plan", h, lp(rel), lp(Hl), lib.iptr(alive))
    call("noplan-shard_download_balanced_offspring", "pk_shard_download_balanced_offspring", h, P, lp(hi))
    call("noplan-shard_pack_balanced_dev", "pk_shard_pack_balanced_dev", h, lp(no_table), 1, 0, buf)
    call("noplan-shard_pack_balanced_loop_dev", "pk_shard_pack_balanced_loop_dev", h, 0, 0, 0, buf)
    for mode in (0, 1, 2):
        call("noplan-shard_adopt_balanced_dev-mode%d" % mode, "pk_shard_adopt_balanced_dev", h, lp(no_table), 1, 0, buf, 0, mode)
    call("args-resample-u=1", "pk_resample", h, 1.0, LINEAR, None)
    call("args-resample-u<0", "pk_resample", h, -0.25, LINEAR, None)
    call("args-resample-u-nan", "pk_resample", h, float("nan"), LINEAR, None)
    call("args-resample-domain=2", "pk_resample", h, 0.5, 2, None)
    call("args-resample-domain=-1", "pk_resample", h, 0.5, -1, None)
    call("args-resample-u=1-and-domain=2", "pk_resample", h, 1.0, 2, None)  # precedence: u first
    call("args-shard_offspring-first-block-beyond", "pk_shard_offspring", h, lib.dptr(totals), 1, 1, P, 0.37, 1, lp(hi))
    call("args-shard_offspring-fewer-global-particles", "pk_shard_offspring", h, lib.dptr(totals), 1, 0, P - 1, 0.37, 1, lp(hi))
    call("args-shard_offspring-u=1", "pk_shard_offspring", h, lib.dptr(totals), 1, 0, P, 1.0, 1, lp(hi))
    call("args-shard_plan_dev-first-block-beyond", "pk_shard_plan_dev", h, buf, 1, 1, P, 0.37, 1, 1, buf)
    call("args-shard_plan_dev-world-times-P", "pk_shard_plan_dev", h, buf, 1, 0, P + 1, 0.37, 1, 1, buf)
    call("args-shard_plan_dev-world=0", "pk_shard_plan_dev", h, buf, 1, 0, P, 0.37, 1, 0, buf)
    call("args-shard_plan_dev-null-ranges", "pk_shard_plan_dev", h, buf, 1, 0, P, 0.37, 1, 1, None)
    call("args-pack_particles-null-buffer", "pk_pack_particles", h, lp(one), 1, None)
    call("args-pack_particles-more-than-P", "pk_pack_particles", h, lp(iota), P + 1, buf)
    call("args-pack_particles-index=P", "pk_pack_particles", h, lp(np.array([P], dtype=np.int64)), 1, buf)
    call("args-pack_particles-none", "pk_pack_particles", h, None, 0, None)  # nothing to pack: accepted
    call("args-adopt_particles-null-src", "pk_adopt_particles", h, None, buf, 0)
    call("args-adopt_particles-src=P", "pk_adopt_particles", h, lp(np.full(P, P, dtype=np.int64)), buf, 0)
    call("args-adopt_particles-src=-1-none-received", "pk_adopt_particles", h, lp(np.full(P, -1, dtype=np.int64)), buf, 0)
    call("args-set_shard-negative", "pk_set_shard", h, -1)
    assert out["noplan-shard_download_offspring"] != "ok"
    host_plan(f)
    call("plan-shard_download_offspring", "pk_shard_download_offspring", h, lp(hi))  # accepted now
    call("plan-shard_adopt_remote_dev-without-local", "pk_shard_adopt_remote_dev", h, 0, buf, 0)
    call("plan-shard_pack_dev-rank=-1", "pk_shard_pack_dev", h, lp(ranges), 1, -1, buf)
    call("plan-shard_pack_dev-rank=world", "pk_shard_pack_dev", h, lp(ranges), 1, 1, buf)
    call("plan-shard_pack_slots_dev-j1-beyond-P", "pk_shard_pack_slots_dev", h, 0, P + 1, 0, P, buf)
    call("plan-shard_pack_slots_dev-null-buffer", "pk_shard_pack_slots_dev", h, 0, 1, 0, P, None)
    call("plan-shard_adopt_dev-records-without-buffer", "pk_shard_adopt_dev", h, 0, None, 1)
    # ---- ... and the balanced placement on the same filter: the contiguous protocol and the plain resample refuse
    f.upload_logical(iota)
    call("balanced-resample", "pk_resample", h, 0.5, LINEAR, None)
    call("balanced-adopt_particles", "pk_adopt_particles", h, lp(iota), buf, 0)
    call("balanced-shard_adopt_dev", "pk_shard_adopt_dev", h, 0, buf, 0)
    call("balanced-shard_adopt_local_dev", "pk_shard_adopt_local_dev", h, 0)
    call("precedence-balanced-and-src-out-of-range-adopt_particles", "pk_adopt_particles", h, lp(np.full(P, P, dtype=np.int64)), buf, 0)
    call("precedence-balanced-and-null-src-adopt_particles", "pk_adopt_particles", h, None, buf, 0)
    call("precedence-balanced-and-u=1-resample", "pk_resample", h, 1.0, LINEAR, None)
    call("precedence-balanced-and-rank=-1-shard_adopt_dev", "pk_shard_adopt_dev", h, -1, buf, 0)
    call("precedence-balanced-and-rank=-1-shard_adopt_local_dev", "pk_shard_adopt_local_dev", h, -1)
    f.close()

    # ---- the balanced placement without a plan: the plan is asked for first
    f = new_filter()
    h = f._h
    f.upload_logical(iota)
    call("precedence-balanced-and-no-plan-shard_adopt_dev", "pk_shard_adopt_dev", h, 0, buf, 0)
    call("precedence-balanced-and-no-plan-shard_adopt_local_dev", "pk_shard_adopt_local_dev", h, 0)
    call("precedence-balanced-and-no-balanced-plan-shard_pack_balanced_dev", "pk_shard_pack_balanced_dev", h, lp(no_table), 1, 0, buf)
    f.close()

    # ---- a growing filter
    f = new_filter()
    h = f._h
    f.grow_enable(L - 4, 64, 30.0)
    assert f.particle_bytes() * P <= SCRATCH_BYTES
    call("grow-pack_particles", "pk_pack_particles", h, lp(one), 1, buf)
    call("grow-adopt_particles", "pk_adopt_particles", h, lp(iota), buf, 0)
    call("grow-shard_pack_dev", "pk_shard_pack_dev", h, lp(ranges), 1, 0, buf)
    call("grow-shard_pack_slots_dev", "pk_shard_pack_slots_dev", h, 0, 0, 0, 0, buf)
    call("grow-shard_adopt_dev", "pk_shard_adopt_dev", h, 0, buf, 0)
    call("grow-shard_adopt_local_dev", "pk_shard_adopt_local_dev", h, 0)
    call("grow-shard_adopt_remote_dev", "pk_shard_adopt_remote_dev", h, 0, buf, 0)
    call("grow-observe_staged_range", "pk_observe_staged_range", h, 0, 0, P, 1, 1)
    call("precedence-grow-and-index-out-of-range-pack_particles", "pk_pack_particles", h, lp(np.array([P], dtype=np.int64)), 1, buf)
    call("precedence-grow-and-null-buffer-pack_particles", "pk_pack_particles", h, lp(one), 1, None)
    call("precedence-grow-and-src-out-of-range-adopt_particles", "pk_adopt_particles", h, lp(np.full(P, P, dtype=np.int64)), buf, 0)
    call("precedence-grow-and-null-src-adopt_particles", "pk_adopt_particles", h, None, buf, 0)
    call("precedence-grow-and-rank=-1-shard_pack_dev", "pk_shard_pack_dev", h, lp(ranges), 1, -1, buf)
    call("precedence-grow-and-null-ranges-shard_pack_dev", "pk_shard_pack_dev", h, None, 1, 0, buf)
    call("precedence-grow-and-bad-range-shard_pack_slots_dev", "pk_shard_pack_slots_dev", h, 0, P + 1, 0, 0, buf)
    call("precedence-grow-and-rank=-1-shard_adopt_dev", "pk_shard_adopt_dev", h, -1, buf, 0)
    call("precedence-grow-and-rank=-1-shard_adopt_local_dev", "pk_shard_adopt_local_dev", h, -1)
    call("precedence-grow-and-rank=-1-shard_adopt_remote_dev", "pk_shard_adopt_remote_dev", h, -1, buf, 0)
    call("precedence-grow-and-no-balanced-plan-shard_adopt_balanced_dev-mode1", "pk_shard_adopt_balanced_dev", h, lp(no_table), 1, 0, buf, 0, 1)
    # a balanced plan of a world of one (uniform weights: every particle keeps its slot), then the adoption in pieces is refused
    call("grow-shard_state_dev", "pk_shard_state_dev", h, state)
    call("grow-shard_plan_balanced_dev", "pk_shard_plan_balanced_dev", h, state, P, None, LINEAR, 0.37, 1, 0, table_dev)
    f.synchronize()
    table = hip.to_host(table_dev, np.int64, 6)
    call("grow-shard_adopt_balanced_dev-mode1", "pk_shard_adopt_balanced_dev", h, lp(table), 1, 0, buf, 0, 1)
    call("grow-shard_adopt_balanced_dev-mode2", "pk_shard_adopt_balanced_dev", h, lp(table), 1, 0, buf, 0, 2)
    call("grow-shard_adopt_balanced_dev-mode3", "pk_shard_adopt_balanced_dev", h, lp(table), 1, 0, buf, 0, 3)
    call("precedence-grow-and-balanced-adopt_particles", "pk_adopt_particles", h, lp(iota), buf, 0)
    f.close()

    # ---- NULL handles: refused by the argument check, whatever comes in front of it
    call("null-set_shard", "pk_set_shard", None, 0)
    call("null-resample", "pk_resample", None, 0.5, LINEAR, None)
    call("null-pack_particles", "pk_pack_particles", None, lp(one), 1, buf)
    call("null-adopt_particles", "pk_adopt_particles", None, lp(iota), buf, 0)
    call("null-shard_pack_dev", "pk_shard_pack_dev", None, lp(ranges), 1, 0, buf)
    call("null-shard_pack_slots_dev", "pk_shard_pack_slots_dev", None, 0, 0, 0, 0, buf)
    call("null-shard_adopt_dev", "pk_shard_adopt_dev", None, 0, buf, 0)
    call("null-shard_adopt_local_dev", "pk_shard_adopt_local_dev", None, 0)
    call("null-shard_adopt_remote_dev", "pk_shard_adopt_remote_dev", None, 0, buf, 0)
    call("null-shard_download_offspring", "pk_shard_download_offspring", None, lp(hi))
    call("null-shard_local_span_dev", "pk_shard_local_span_dev", None, buf)
    call("null-shard_pack_balanced_dev", "pk_shard_pack_balanced_dev", None, lp(no_table), 1, 0, buf)
    call("null-shard_pack_balanced_loop_dev", "pk_shard_pack_balanced_loop_dev", None, 0, 0, 0, buf)
    call("null-shard_adopt_balanced_dev", "pk_shard_adopt_balanced_dev", None, lp(no_table), 1, 0, buf, 0, 0)
    hip.free_all()
    return out


def record_scan(lib):
    """The scan-taking calls' argument refusals, every case in order: name -> "ok" | [status, message]."""
    abi = lib.load()
    out = {}
    dp, ip = lib.dptr, lib.iptr
    good = np.array([[0.3, 20.0, 50.0, 90.0], [-0.2, 200.0, 50.0, 90.0]])
    nan1 = good.copy()
    nan1[1, 2] = np.nan  # blob 1, double 6
    many = np.tile(good, (32768, 1))  # 65 536 blobs
    ids_out = np.zeros(P * 2, dtype=np.int32)
    delta, alpha = np.array([0.01, 0.05, 0.0]), np.array([0.01, 0.01, 0.01, 0.01])

    def ids(a, b):
        return np.array([a, b], dtype=np.int32)

    # call -> (takes ids, fn(handle, blobs, B, ids))
    calls = {
        "observe": (True, lambda h, b, B, i: abi.pk_observe(h, dp(b), B, ip(i), None)),
        "observe_fresh": (True, lambda h, b, B, i: abi.pk_observe_fresh(h, dp(b), B, ip(i), None)),
        "associate": (False, lambda h, b, B, i: abi.pk_associate(h, dp(b), B, ip(ids_out))),
        "stage_scan": (False, lambda h, b, B, i: abi.pk_stage_scan(h, dp(b), B)),
        "step": (True, lambda h, b, B, i: abi.pk_step(h, 0.1, 0.02, 0.1, None, 5, 0, dp(b), B, ip(i), 0.37, LINEAR)),
        "propose": (True, lambda h, b, B, i: abi.pk_propose(h, 0.1, 0.02, 0.1, None, 5, 0, dp(b), B, ip(i), 0, None)),
        "propose_odom": (True, lambda h, b, B, i: abi.pk_propose_odom(h, dp(delta), dp(alpha), None, 5, 0, dp(b), B, ip(i), 0, None)),
    }

    def new_filter(name, with_map=True):
        f = lib.DeviceFilter(P, L)
        if with_map:
            means = np.column_stack([np.linspace(-4.0, 4.0, L), np.linspace(3.0, 5.0, L), np.linspace(10.0, 220.0, L), np.full(L, 50.0), np.full(L, 90.0)])
            f.upload_map(means, np.tile(0.25 * np.identity(5), (L, 1, 1)).reshape(L, 25))
        poses = np.zeros((P, 4))
        poses[:, 3] = 1.0
        f.upload_poses(poses)
        if name.startswith("propose"):
            f.set_measurement_model("bearing")
        return f

    for name, (takes_ids, fn) in calls.items():
        def call(case, h, b, B, i=None):
            assert name + "-" + case not in out, case
            st = fn(h, b, B, i)
            out[name + "-" + case] = "ok" if st == lib.PK_OK else [int(st), abi.pk_last_error().decode()]

        f = new_filter(name, with_map=False)
        call("no-map", f._h, good, 2)
        call("no-map-and-nan", f._h, nan1, 2)
        call("no-map-and-negative-B", f._h, good, -1)
        f.close()
        f = new_filter(name)
        h = f._h
        call("negative-B", h, good, -1)
        call("null-blobs", h, None, 2)
        call("nan-in-blob-1", h, nan1, 2)
        f.scan_ranges(np.array([2.0, np.nan, 3.0]), np.array([0.01, 0.0, 0.02]))  # named for a scan of three blobs
        call("ranges-of-3-blobs-and-nan", h, nan1, 2)
        if takes_ids:
            call("ids=-1", h, good, 2, ids(1, -1))
            call("ids=L+1", h, good, 2, ids(L + 1, 1))
            call("nan-and-ids=L+1", h, nan1, 2, ids(L + 1, 1))
            call("null-blobs-and-ids=L+1", h, None, 2, ids(L + 1, 1))
            call("ids=L", h, good, 2, ids(L, 1))
        call("B=0", h, None, 0)
        if name == "associate":
            assert "associate-null-ids_out" not in out
            st = abi.pk_associate(h, dp(good), 2, None)
            out["associate-null-ids_out"] = "ok" if st == lib.PK_OK else [int(st), abi.pk_last_error().decode()]
        if name in ("observe", "propose"):
            call("65536-blobs", h, many, 65536)
        if name == "propose":
            f.set_measurement_model("reference")
            call("reference-model-and-negative-B", h, good, -1)
            call("reference-model-and-null-blobs", h, None, 2)
        f.close()
        if takes_ids:  # a growing filter: supplied ids are refused (the proposal: once pk_proposal_grow lets it run there at all)
            f = new_filter(name)
            f.grow_enable(L - 4, 64, 30.0)
            call("grow-and-ids", f._h, good, 2, ids(1, 0))
            if name.startswith("propose"):
                f.proposal_grow(True)
                call("proposal_grow-and-ids", f._h, good, 2, ids(1, 0))
                call("proposal_grow-and-ids-and-nan", f._h, nan1, 2, ids(1, 0))
            call("grow-and-ids-and-B=0", f._h, None, 0, ids(1, 0))
            f.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def answers(lib):
    return record(lib)


def test_the_cases_are_the_fixtures(golden, answers):
    assert sorted(golden) == sorted(answers)


def test_no_case_is_a_runtime_error(golden):
    """A HIP error's message ends in a source position, which is no part of the contract: none is recorded."""
    assert not [k for k, v in golden.items() if v != "ok" and (v[0] in (-2, -5) or "failed:" in v[1])]


def test_every_option_is_refused_outside_its_range_only(golden):
    for name, rng in OPTIONS.items():
        values = (-5, 7, 1, 0) if rng is None else (rng[0] - 1, rng[1] + 1, rng[1], rng[0])
        got = [golden["option-%s=%d" % (name, v)] for v in values]
        assert got[2:] == ["ok", "ok"], name
        if rng is None:
            assert got[:2] == ["ok", "ok"], name
        else:
            assert got[0] != "ok" and got[0] == got[1] and got[0][0] == -1 and got[0][1].startswith(name + ":"), name


def test_every_call_is_answered_as_it_was(golden, answers):
    assert {k: v for k, v in answers.items() if golden.get(k) != v} == {}


@pytest.fixture(scope="module")
def scan_golden():
    with open(SCAN_FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def scan_answers(lib):
    return record_scan(lib)


def test_the_scan_cases_are_the_fixtures(scan_golden, scan_answers):
    assert sorted(scan_golden) == sorted(scan_answers)
    assert not [k for k, v in scan_golden.items() if v != "ok" and (v[0] in (-2, -5) or "failed:" in v[1])]  # (no runtime error)


def test_the_scan_fixture_shows_what_it_is_for(scan_golden):
    g = scan_golden
    for call in ("observe", "observe_fresh", "associate", "stage_scan", "step", "propose", "propose_odom"):
        assert g[call + "-nan-in-blob-1"][1].endswith("blob 1 is not finite"), call
        assert "no map uploaded" in g[call + "-no-map"][1] and g[call + "-no-map-and-nan"] == g[call + "-no-map"], call
        assert "pk_scan_ranges named the ranges of a scan of 3 blobs" in g[call + "-ranges-of-3-blobs-and-nan"][1] or call.startswith("propose"), call
        assert g[call + "-B=0"] == ("ok" if call != "stage_scan" else g["stage_scan-negative-B"]), call
    for call in ("observe", "observe_fresh", "step", "propose", "propose_odom"):
        assert g[call + "-ids=L"] == "ok" and g[call + "-ids=-1"][1].endswith("ids[1] = -1 outside 0..%d" % L), call
        assert g[call + "-ids=L+1"][1].endswith("ids[0] = %d outside 0..%d" % (L + 1, L)), call
        assert g[call + "-nan-and-ids=L+1"] == g[call + "-nan-in-blob-1"], call  # the values before the ids
    assert g["propose-proposal_grow-and-ids-and-nan"] == g["propose-proposal_grow-and-ids"]  # the proposal: no ids before bad values
    assert g["propose-reference-model-and-negative-B"] == g["propose-reference-model-and-null-blobs"]  # the proposal's own refusals first
    assert g["observe-65536-blobs"] != "ok" and g["propose-65536-blobs"] != "ok" and g["associate-null-ids_out"] != "ok"


def test_every_scan_call_is_answered_as_it_was(scan_golden, scan_answers):
    assert {k: v for k, v in scan_answers.items() if scan_golden.get(k) != v} == {}


if __name__ == "__main__":
    from parakeet_slam_amd import _lib

    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    differ = 0
    for path, rec in ((FIXTURE, record), (SCAN_FIXTURE, record_scan)):
        got = rec(_lib)
        if "--record" in sys.argv:
            with open(path, "w") as fh:
                fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(got[k])) for k in sorted(got)) + "\n}\n")
            print("recorded %d cases from %s in %s" % (len(got), _lib.LIB_PATH, os.path.basename(path)))
        else:
            with open(path) as fh:
                want = json.load(fh)
            bad = [k for k in sorted(set(want) | set(got)) if got.get(k) != want.get(k)]
            print("%s: %d cases, %d differ from the fixture: %s" % (os.path.basename(path), len(got), len(bad), bad))
            differ += len(bad)
    sys.exit(1 if differ else 0)

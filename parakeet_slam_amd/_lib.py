"""ctypes binding of ``libparakeet_slam.so`` (include/parakeet_slam.h).

The library is the product path.  There is no CPU fallback: if the shared object
is missing, or no HIP device is visible when a filter is created, this fails
loudly (``PkError`` / ``OSError``) instead of computing anything on the host.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import adaptive, mapsum, path

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libparakeet_slam.so")

PK_OK = 0
PK_ERR_INVALID, PK_ERR_HIP, PK_ERR_STATE, PK_ERR_UNSUPPORTED, PK_ERR_NOMEM = -1, -2, -3, -4, -5
PK_WEIGHTS_LINEAR, PK_WEIGHTS_LOG = 0, 1
PK_PATH_UNIFORM = 2  # pk_path_settle's third weighting: every current particle counts once
PK_MAP_UNIFORM, PK_MAP_WEIGHTED = mapsum.UNIFORM, mapsum.WEIGHTED
PK_LANDMARK_POTENTIAL = 0x40000000  # flag in a landmark's count word: potential feature (prkt_core_v2.py:109-118)
PK_GROW_VIEW_STATS_BYTES = 32  # pk_grow_view's counters on the device (include/parakeet_slam.h)
PK_T_NAMES = ("motion", "assoc", "observe", "weights", "resample", "summary", "materialise", "propose")
PK_T_COUNT = len(PK_T_NAMES)
PK_PROBE_LEN = 79
(PK_MATH_LOG_FEW_ULP, PK_MATH_PUB_LOG, PK_MATH_PUB_RECIP, PK_MATH_ATAN2, PK_MATH_ROUND_DOWN_F32, PK_MATH_KEY, PK_MATH_FAR_BOUND,
 PK_MATH_PR_FROM_PARTS) = range(8)
PK_MATH_EKF_UPDATE, PK_MATH_MATCH = 9, 10  # (8 stays refused: parakeet_slam.h)
PK_MATH_SHAPES = {PK_MATH_LOG_FEW_ULP: (1, 1), PK_MATH_PUB_LOG: (1, 1), PK_MATH_PUB_RECIP: (1, 1), PK_MATH_ATAN2: (2, 1),
                  PK_MATH_ROUND_DOWN_F32: (1, 1), PK_MATH_KEY: (1, 2), PK_MATH_FAR_BOUND: (14, 2), PK_MATH_PR_FROM_PARTS: (4, 1),
                  PK_MATH_EKF_UPDATE: (31, 17), PK_MATH_MATCH: (23, 5)}  # op -> (arity, outputs)
PK_ABI_VERSION = 1
PK_MODEL_REFERENCE, PK_MODEL_BEARING = 0, 1  # pk_set_measurement_model
MEASUREMENT_MODELS = {"reference": PK_MODEL_REFERENCE, "bearing": PK_MODEL_BEARING}
PK_BEARING_SHAPES = {0: (23, 5), 1: (32, 17)}  # pk_probe_bearing: what -> (arity, outputs)
PK_RANGE_SHAPES = {0: (26, 5), 1: (33, 16)}    # pk_probe_range: what -> (arity, outputs)
PK_GROW_INIT_REFERENCE, PK_GROW_INIT_TRIANGULATED = 0, 1  # pk_grow_init
LANDMARK_INITS = {"reference": PK_GROW_INIT_REFERENCE, "triangulated": PK_GROW_INIT_TRIANGULATED}


def measurement_model_code(model):
    """The PK_MODEL_* value of a model's name ("reference", "bearing") or of the value itself; ValueError for anything else."""
    if isinstance(model, str):
        if model not in MEASUREMENT_MODELS:
            raise ValueError("measurement_model: %r is neither %s" % (model, " nor ".join(repr(k) for k in MEASUREMENT_MODELS)))
        return MEASUREMENT_MODELS[model]
    return int(model)


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_bp = C.POINTER(C.c_uint8)
_up = C.POINTER(C.c_uint32)
_h = C.c_void_p

# name -> (restype, argtypes); mirrors include/parakeet_slam.h one to one
SIGNATURES = {
    "pk_abi_version": (C.c_int, []),
    "pk_status_string": (C.c_char_p, [C.c_int]),
    "pk_last_error": (C.c_char_p, []),
    "pk_device_count": (C.c_int, []),
    "pk_create": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(_h)]),
    "pk_destroy": (C.c_int, [_h]),
    "pk_set_stream": (C.c_int, [_h, C.c_void_p]),
    "pk_synchronize": (C.c_int, [_h]),
    "pk_num_particles": (C.c_int64, [_h]),
    "pk_num_landmarks": (C.c_int32, [_h]),
    "pk_device_bytes": (C.c_int64, [_h]),
    "pk_set_option": (C.c_int, [_h, C.c_char_p, C.c_int64]),
    "pk_set_measurement_noise": (C.c_int, [_h, _dp]),
    "pk_set_measurement_model": (C.c_int, [_h, C.c_int32]),
    "pk_measurement_model": (C.c_int, [_h, C.POINTER(C.c_int32)]),
    "pk_upload_map": (C.c_int, [_h, _dp, _dp, _bp]),
    "pk_upload_poses": (C.c_int, [_h, _dp]),
    "pk_download_poses": (C.c_int, [_h, _dp]),
    "pk_upload_pose": (C.c_int, [_h, C.c_int64, _dp]),
    "pk_download_landmarks": (C.c_int, [_h, C.c_int64, C.c_int64, _dp, _dp, _ip]),
    "pk_upload_landmarks": (C.c_int, [_h, C.c_int64, C.c_int64, _dp, _dp, _ip]),
    "pk_reset_weights": (C.c_int, [_h]),
    "pk_motion": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_uint64, C.c_uint64]),
    "pk_download_log_weights": (C.c_int, [_h, _dp]),
    "pk_upload_log_weights": (C.c_int, [_h, _dp]),
    "pk_observe": (C.c_int, [_h, _dp, C.c_int32, _ip, _ip]),
    "pk_observe_fresh": (C.c_int, [_h, _dp, C.c_int32, _ip, _ip]),
    "pk_stage_scan": (C.c_int, [_h, _dp, C.c_int32]),
    "pk_observe_staged": (C.c_int, [_h, C.c_int32]),
    "pk_associate": (C.c_int, [_h, _dp, C.c_int32, _ip]),
    "pk_resample": (C.c_int, [_h, C.c_double, C.c_int32, _lp]),
    "pk_summary": (C.c_int, [_h, _dp]),
    "pk_pose_sums": (C.c_int, [_h, _dp]),
    "pk_map_moments": (C.c_int, [_h, C.c_int32, C.c_double, _dp, _dp, _dp, _dp, _dp]),
    "pk_map_summary": (C.c_int, [_h, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
    "pk_map_match_moments": (C.c_int, [_h, C.c_int32, C.c_double, _dp, C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "pk_map_discovered": (C.c_int, [_h, C.c_int32, C.c_int64, C.c_double, C.c_double, _lp, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp,
                                    _dp, _dp]),
    "pk_path_enable": (C.c_int, [_h, C.c_int32]),
    "pk_path_shape": (C.c_int, [_h, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pk_path_download": (C.c_int, [_h, C.c_int32, C.c_int32, _dp, _ip]),
    "pk_path_upload": (C.c_int, [_h, C.c_int32, C.c_int64, _dp, _ip]),
    "pk_path_trace": (C.c_int, [_h, _lp, C.c_int64, _dp]),
    "pk_path_summary": (C.c_int, [_h, _dp, _dp, _lp]),
    "pk_path_summary_weighted": (C.c_int, [_h, C.c_int32, _dp, _dp, _dp]),
    "pk_path_trunk_enable": (C.c_int, [_h, C.c_int32]),
    "pk_path_settle": (C.c_int, [_h, C.c_int32, C.c_int32]),
    "pk_path_trunk_shape": (C.c_int, [_h, C.POINTER(C.c_int32), _lp, _lp]),
    "pk_path_trunk_download": (C.c_int, [_h, C.c_int64, C.c_int64, _dp]),
    "pk_path_trunk_upload": (C.c_int, [_h, C.c_int64, C.c_int64, _dp]),
    "pk_path_trunk_summary": (C.c_int, [_h, C.c_int64, C.c_int64, _dp, _dp, _lp]),
    "pk_best_particle": (C.c_int, [_h, _lp, _dp]),
    "pk_step": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_uint64, C.c_uint64, _dp, C.c_int32,
                          _ip, C.c_double, C.c_int32]),
    "pk_resample_adaptive": (C.c_int, [_h, C.c_double, C.c_int32, C.c_double, _lp]),
    "pk_step_adaptive": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_uint64, C.c_uint64, _dp, C.c_int32,
                                   _ip, C.c_double, C.c_int32, C.c_double]),
    "pk_resample_stats": (C.c_int, [_h, _dp, C.POINTER(C.c_int32), _lp]),
    "pk_weight_sums": (C.c_int, [_h, C.c_int32, C.c_double, _dp]),
    "pk_summary_weighted": (C.c_int, [_h, C.c_int32, _dp, _dp, _dp]),
    "pk_odom_delta": (C.c_int, [_dp, _dp, C.c_double, _dp]),
    "pk_odom_sigmas": (C.c_int, [_dp, _dp, _dp]),
    "pk_motion_odom": (C.c_int, [_h, _dp, _dp, _dp, C.c_uint64, C.c_uint64]),
    "pk_propose": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, _dp, C.c_uint64, C.c_uint64, _dp, C.c_int32, _ip, C.c_int32, _ip]),
    "pk_propose_odom": (C.c_int, [_h, _dp, _dp, _dp, C.c_uint64, C.c_uint64, _dp, C.c_int32, _ip, C.c_int32, _ip]),
    "pk_proposal_download": (C.c_int, [_h, _dp, _dp, _ip]),
    "pk_proposal_ranges": (C.c_int, [_h, C.c_int32]),
    "pk_proposal_ranges_state": (C.c_int, [_h, C.POINTER(C.c_int32)]),
    "pk_proposal_grow": (C.c_int, [_h, C.c_int32]),
    "pk_proposal_grow_state": (C.c_int, [_h, C.POINTER(C.c_int32)]),
    "pk_assoc_unique": (C.c_int, [_h, C.c_int32]),
    "pk_assoc_unique_state": (C.c_int, [_h, C.POINTER(C.c_int32)]),
    "pk_assoc_unique_stats": (C.c_int, [_h, _lp]),
    "pk_motion_odom_range": (C.c_int, [_h, _dp, _dp, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64]),
    "pk_step_odom": (C.c_int, [_h, _dp, _dp, _dp, C.c_uint64, C.c_uint64, _dp, C.c_int32, _ip, C.c_double, C.c_int32, C.c_double]),
    "pk_shard_max_logw": (C.c_int, [_h, _dp]),
    "pk_shard_num_blocks": (C.c_int64, [_h]),
    "pk_shard_block_totals": (C.c_int, [_h, C.c_double, C.c_int32, _dp]),
    "pk_set_shard": (C.c_int, [_h, C.c_int64]),
    "pk_shard_offspring": (C.c_int, [_h, _dp, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int32, _lp]),
    "pk_shard_max_logw_dev": (C.c_int, [_h, C.c_void_p]),
    "pk_shard_block_totals_dev": (C.c_int, [_h, C.c_void_p, C.c_int32, C.c_void_p]),
    "pk_shard_plan_dev": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int32, C.c_int32,
                                    C.c_void_p]),
    "pk_shard_logw_dev": (C.c_int, [_h, C.c_void_p]),
    "pk_shard_plan_global_dev": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                           C.c_void_p]),
    "pk_shard_download_offspring": (C.c_int, [_h, _lp]),
    "pk_shard_pack_dev": (C.c_int, [_h, _lp, C.c_int32, C.c_int32, C.c_void_p]),
    "pk_shard_pack_slots_dev": (C.c_int, [_h, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "pk_shard_adopt_dev": (C.c_int, [_h, C.c_int32, C.c_void_p, C.c_int64]),
    "pk_shard_local_span_dev": (C.c_int, [_h, C.c_void_p]),
    "pk_shard_adopt_local_dev": (C.c_int, [_h, C.c_int32]),
    "pk_shard_adopt_remote_dev": (C.c_int, [_h, C.c_int32, C.c_void_p, C.c_int64]),
    "pk_shard_state_dev": (C.c_int, [_h, C.c_void_p]),
    "pk_shard_plan_balanced_dev": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                             C.c_void_p]),
    "pk_shard_pack_balanced_dev": (C.c_int, [_h, _lp, C.c_int32, C.c_int32, C.c_void_p]),
    "pk_shard_adopt_balanced_dev": (C.c_int, [_h, _lp, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32]),
    "pk_shard_pack_balanced_loop_dev": (C.c_int, [_h, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "pk_shard_download_logical": (C.c_int, [_h, _lp]),
    "pk_shard_reset_placement": (C.c_int, [_h]),
    "pk_shard_upload_logical": (C.c_int, [_h, _lp]),
    "pk_shard_download_balanced_plan": (C.c_int, [_h, _lp, _lp, _ip]),
    "pk_shard_download_balanced_offspring": (C.c_int, [_h, C.c_int64, _lp]),
    "pk_shard_balanced_errors": (C.c_int, [_h, _lp]),
    "pk_motion_range": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64]),
    "pk_staged_takes_regs": (C.c_int, [_h]),
    "pk_observe_staged_range": (C.c_int, [_h, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "pk_particle_bytes": (C.c_int64, [_h]),
    "pk_pack_particles": (C.c_int, [_h, _lp, C.c_int64, C.c_void_p]),
    "pk_adopt_particles": (C.c_int, [_h, _lp, C.c_void_p, C.c_int64]),
    "pk_probe": (C.c_int, [C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]),
    "pk_probe_math": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _dp, _dp]),
    "pk_probe_bearing": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _dp, _dp]),
    "pk_probe_range": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _dp, _dp]),
    "pk_scan_ranges": (C.c_int, [_h, _dp, _dp, C.c_int32]),
    "pk_scan_ranges_state": (C.c_int, [_h, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pk_enable_timing": (C.c_int, [_h, C.c_int32]),
    "pk_reset_timings": (C.c_int, [_h]),
    "pk_timings": (C.c_int, [_h, _dp, _lp]),
    "pk_observe_bytes": (C.c_int, [_h, C.c_int32, _lp, _lp]),
    "pk_colour_table_stats": (C.c_int, [_h, _lp]),
    "pk_observe_route": (C.c_int, [_h]),
    "pk_download_sources": (C.c_int, [_h, _ip]),
    "pk_observe_flagged": (C.c_int, [_h, _lp, _lp]),
    "pk_observe_retry_rows": (C.c_int, [_h, _lp, _lp]),
    "pk_grow_enable": (C.c_int, [_h, C.c_int32, C.c_int32, C.c_double]),
    "pk_grow_download": (C.c_int, [_h, C.c_int64, C.c_int64, _ip, _dp, _ip]),
    "pk_grow_upload": (C.c_int, [_h, C.c_int64, C.c_int64, _ip, _dp, _ip]),
    "pk_grow_shape": (C.c_int, [_h, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pk_grow_init": (C.c_int, [_h, C.c_int32, C.c_double]),
    "pk_grow_init_mode": (C.c_int, [_h, C.POINTER(C.c_int32), _dp]),
    "pk_grow_ranges": (C.c_int, [_h, C.c_int32]),
    "pk_grow_ranges_state": (C.c_int, [_h, C.POINTER(C.c_int32)]),
    "pk_grow_retire": (C.c_int, [_h, C.c_int32, C.c_int32]),
    "pk_grow_clocks_download": (C.c_int, [_h, C.c_int64, C.c_int64, _ip, _up, _ip, _ip, _up]),
    "pk_grow_clocks_upload": (C.c_int, [_h, C.c_int64, C.c_int64, _ip, _up, _ip, _ip, _up]),
    "pk_grow_view": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, C.c_int32]),
    "pk_grow_view_state": (C.c_int, [_h, C.POINTER(C.c_int32), _dp, C.POINTER(C.c_int32)]),
    "pk_grow_view_stats": (C.c_int, [_h, _lp]),
    "pk_observe_published": (C.c_int, [_h, C.POINTER(C.c_int32)]),
    "pk_observe_flags": (C.c_int, [_h, _bp]),
    "pk_observe_pub_stats": (C.c_int, [_h, _lp]),
    "pk_observe_lean_stats": (C.c_int, [_h, _lp]),
    "pk_rng_create_numpy": (C.c_int, [C.c_uint32, C.POINTER(_h)]),
    "pk_rng_create_python": (C.c_int, [C.c_uint32, C.POINTER(_h)]),
    "pk_rng_destroy": (C.c_int, [_h]),
    "pk_rng_standard_normal": (C.c_int, [_h, C.c_int64, _dp]),
    "pk_rng_random": (C.c_int, [_h, C.c_int64, _dp]),
}


class PkError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("parakeet_slam [%d]: %s" % (status, message))
        self.status = status


_lib = None


def load():
    """Load the shared library (once).  Raises OSError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(
            "%s is missing: build it with `python -m parakeet_slam_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the particle update." % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    ver = lib.pk_abi_version()
    if ver != PK_ABI_VERSION:
        raise OSError("libparakeet_slam.so has ABI %d, the binding expects %d: rebuild" % (ver, PK_ABI_VERSION))
    _lib = lib
    return lib


def check(status):
    if status != PK_OK:
        lib = load()
        msg = lib.pk_last_error().decode("utf-8", "replace") or lib.pk_status_string(status).decode()
        raise PkError(status, msg)


def dptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def iptr(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def lptr(a):
    return a.ctypes.data_as(_lp) if a is not None else None


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def odom_delta(prev, now, min_trans=0.01):
    """(rot1, trans, rot2) between two odometry poses (x, y, heading): pk_odom_delta.  Host only, needs no GPU."""
    a, b, out = f64(prev, (3,)), f64(now, (3,)), np.empty(3, dtype=np.float64)
    check(load().pk_odom_delta(dptr(a), dptr(b), float(min_trans), dptr(out)))
    return out


def odom_sigmas(delta, alphas):
    """(sigma_rot1, sigma_trans, sigma_rot2) of a delta under the four noise parameters: pk_odom_sigmas.  Host only."""
    d, a, out = f64(delta, (3,)), f64(alphas, (4,)), np.empty(3, dtype=np.float64)
    check(load().pk_odom_sigmas(dptr(d), dptr(a), dptr(out)))
    return out


class DeviceFilter(object):
    """Thin, numpy-in / numpy-out wrapper of one ``pk_filter`` handle.

    This is the layer the FastSLAM facade, the parity tests and bench.py share.
    """

    def __init__(self, num_particles, num_landmarks, device=0):
        self._lib = load()
        self._h = _h()
        check(self._lib.pk_create(int(num_particles), int(num_landmarks), int(device), C.byref(self._h)))
        self.P = int(num_particles)
        self.L = int(num_landmarks)
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.pk_destroy(self._h)
            self._h = _h()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ---------------------------------------------------
    def set_stream(self, stream_ptr):
        check(self._lib.pk_set_stream(self._h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        check(self._lib.pk_synchronize(self._h))

    def device_bytes(self):
        return int(self._lib.pk_device_bytes(self._h))

    def set_option(self, name, value):
        check(self._lib.pk_set_option(self._h, name.encode(), int(value)))

    def set_measurement_noise(self, Qt):
        q = f64(Qt, (16,))
        check(self._lib.pk_set_measurement_noise(self._h, dptr(q)))

    def set_measurement_model(self, model):
        """"reference" (default) or "bearing" -- or PK_MODEL_* -- for the observes that follow (pk_set_measurement_model)."""
        check(self._lib.pk_set_measurement_model(self._h, measurement_model_code(model)))

    def measurement_model(self):
        m = C.c_int32()
        check(self._lib.pk_measurement_model(self._h, C.byref(m)))
        return {v: k for k, v in MEASUREMENT_MODELS.items()}[int(m.value)]

    def scan_ranges(self, ranges, variances=None):
        """Name the ranges of the NEXT scan (pk_scan_ranges; bearing model): ``ranges[B]`` (NaN = this blob has none) and
        ``variances[B]``; the next call that takes blobs consumes them.  ``None`` or an empty array disarms."""
        if ranges is None or np.size(ranges) == 0:
            check(self._lib.pk_scan_ranges(self._h, None, None, 0))
            return
        r = f64(ranges, (-1,))
        v = None if variances is None else f64(variances, (r.shape[0],))
        check(self._lib.pk_scan_ranges(self._h, dptr(r), None if v is None else dptr(v), r.shape[0]))

    def scan_ranges_state(self):
        """(armed, staged): the number of blobs of the armed ranges and of a staged scan that was given ranges; 0 = none."""
        a, st = C.c_int32(), C.c_int32()
        check(self._lib.pk_scan_ranges_state(self._h, C.byref(a), C.byref(st)))
        return int(a.value), int(st.value)

    def upload_map(self, means, covs, immutable=None):
        m = f64(means, (self.L, 5))
        c = f64(covs, (self.L, 25))
        im = None
        if immutable is not None:
            im = np.ascontiguousarray(immutable, dtype=np.uint8).reshape(self.L)
        check(self._lib.pk_upload_map(self._h, dptr(m), dptr(c), im.ctypes.data_as(_bp) if im is not None else None))

    def upload_poses(self, xyhw):
        a = f64(xyhw, (self.P, 4))
        check(self._lib.pk_upload_poses(self._h, dptr(a)))

    def upload_pose(self, p, xyhw):
        """One particle's (x, y, heading, weight); the other particles keep their log-weights bit for bit."""
        a = f64(xyhw, (4,))
        check(self._lib.pk_upload_pose(self._h, int(p), dptr(a)))

    def download_poses(self):
        out = np.empty((self.P, 4), dtype=np.float64)
        check(self._lib.pk_download_poses(self._h, dptr(out)))
        return out

    def download_landmarks(self, p0=0, p1=None, means=True, covs=True, counts=True):
        p1 = self.P if p1 is None else p1
        n = p1 - p0
        m = np.empty((n, self.L, 5)) if means else None
        c = np.empty((n, self.L, 5, 5)) if covs else None
        k = np.empty((n, self.L), dtype=np.int32) if counts else None
        check(self._lib.pk_download_landmarks(self._h, p0, p1, dptr(m), dptr(c), iptr(k)))
        return m, c, k

    def upload_landmarks(self, p0, p1, means=None, covs=None, counts=None):
        n = p1 - p0
        m = f64(means, (n, self.L, 5)) if means is not None else None
        c = f64(covs, (n, self.L, 25)) if covs is not None else None
        k = np.ascontiguousarray(counts, dtype=np.int32).reshape(n, self.L) if counts is not None else None
        check(self._lib.pk_upload_landmarks(self._h, p0, p1, dptr(m), dptr(c), iptr(k)))

    # -- the step ----------------------------------------------------------
    def reset_weights(self):
        check(self._lib.pk_reset_weights(self._h))

    def motion(self, v, w, dt, z=None, seed=0, draw=0):
        zz = f64(z, (self.P, 3)) if z is not None else None
        check(self._lib.pk_motion(self._h, float(v), float(w), float(dt), dptr(zz), int(seed), int(draw)))

    def motion_odom(self, delta, alphas, z=None, seed=0, draw=0):
        """motion for an odometry delta (rot1, trans, rot2) with the noise parameters (a1, a2, a3, a4): pk_motion_odom."""
        d, a = f64(delta, (3,)), f64(alphas, (4,))
        zz = f64(z, (self.P, 3)) if z is not None else None
        check(self._lib.pk_motion_odom(self._h, dptr(d), dptr(a), dptr(zz), int(seed), int(draw)))

    def propose(self, v, w, dt, blobs, z=None, seed=0, draw=0, ids=None, return_ids=False, fresh=False):
        """One motion(v, w, dt, z, seed, draw) plus one observe(blobs, ids) with every pose drawn from the motion model conditioned
        on the scan (FastSLAM 2.0; bearing model only): pk_propose."""
        b = f64(blobs).reshape(-1, 4)
        B = b.shape[0]
        zz = f64(z, (self.P, 3)) if z is not None else None
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(B) if ids is not None else None
        out = np.empty((self.P, B), dtype=np.int32) if return_ids else None
        check(self._lib.pk_propose(self._h, float(v), float(w), float(dt), dptr(zz), int(seed), int(draw), dptr(b), B, iptr(i),
                                   1 if fresh else 0, iptr(out)))
        return out

    def propose_odom(self, delta, alphas, blobs, z=None, seed=0, draw=0, ids=None, return_ids=False, fresh=False):
        """propose for an odometry delta (rot1, trans, rot2) with the noise parameters (a1, a2, a3, a4): pk_propose_odom."""
        d, a = f64(delta, (3,)), f64(alphas, (4,))
        b = f64(blobs).reshape(-1, 4)
        B = b.shape[0]
        zz = f64(z, (self.P, 3)) if z is not None else None
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(B) if ids is not None else None
        out = np.empty((self.P, B), dtype=np.int32) if return_ids else None
        check(self._lib.pk_propose_odom(self._h, dptr(d), dptr(a), dptr(zz), int(seed), int(draw), dptr(b), B, iptr(i),
                                        1 if fresh else 0, iptr(out)))
        return out

    def proposal_download(self):
        """(xi (P, 3), dlogw (P,), used (P,)) of the last propose / propose_odom: pk_proposal_download."""
        xi, dl, used = np.empty((self.P, 3)), np.empty(self.P), np.empty(self.P, dtype=np.int32)
        check(self._lib.pk_proposal_download(self._h, dptr(xi), dptr(dl), iptr(used)))
        return xi, dl, used

    def proposal_ranges(self, on=True):
        """Ranges in the proposal (pk_proposal_ranges): on, propose / propose_odom consume the ranges scan_ranges armed -- a ranged
        blob enters the sampling, the weight and the update as a (bearing, range) measurement -- instead of refusing them."""
        check(self._lib.pk_proposal_ranges(self._h, 1 if on else 0))

    def proposal_ranges_state(self):
        """Whether propose / propose_odom take armed ranges: pk_proposal_ranges_state."""
        on = C.c_int32(0)
        check(self._lib.pk_proposal_ranges_state(self._h, C.byref(on)))
        return bool(on.value)

    def proposal_grow(self, on=True):
        """The proposal on growing maps (pk_proposal_grow): on, propose / propose_odom run on a filter with grow_enable / grow_retire
        -- the new-landmark bookkeeping and retirement follow the step at the sampled poses -- instead of refusing it."""
        check(self._lib.pk_proposal_grow(self._h, int(on)))

    def proposal_grow_state(self):
        """Whether propose / propose_odom run on a growing filter: pk_proposal_grow_state."""
        on = C.c_int32(0)
        check(self._lib.pk_proposal_grow_state(self._h, C.byref(on)))
        return bool(on.value)

    def assoc_unique(self, on=True):
        """Unique association (pk_assoc_unique): on, every maximum-likelihood scan's ids are settled so that at most one blob keeps
        each landmark of a particle -- the greedy matching by (probability descending, blob ascending, landmark ascending)."""
        check(self._lib.pk_assoc_unique(self._h, int(on)))

    def assoc_unique_state(self):
        """Whether unique association is on: pk_assoc_unique_state."""
        on = C.c_int32(0)
        check(self._lib.pk_assoc_unique_state(self._h, C.byref(on)))
        return bool(on.value)

    def assoc_unique_stats(self):
        """Of the last scan settled in the mode (pk_assoc_unique_stats; synchronises): particles with a conflict, blobs whose id
        changed, of those the ones matched to another landmark, the most passes any particle took.  int64[4]."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.pk_assoc_unique_stats(self._h, out.ctypes.data_as(_lp)))
        return out

    def download_log_weights(self):
        out = np.empty(self.P, dtype=np.float64)
        check(self._lib.pk_download_log_weights(self._h, dptr(out)))
        return out

    def upload_log_weights(self, logw):
        """Every particle's log-weight, bit for bit (upload_poses takes log(weight): exp and log do not round-trip)."""
        a = f64(logw, (self.P,))
        check(self._lib.pk_upload_log_weights(self._h, dptr(a)))

    def observe(self, blobs, ids=None, return_ids=False, fresh=False):
        """fresh: the weights restart from 1 first (prkt_core_v2.py:73), fused into the same kernels."""
        b = f64(blobs).reshape(-1, 4)
        B = b.shape[0]
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(B) if ids is not None else None
        out = np.empty((self.P, B), dtype=np.int32) if return_ids else None
        fn = self._lib.pk_observe_fresh if fresh else self._lib.pk_observe
        check(fn(self._h, dptr(b), B, iptr(i), iptr(out)))
        return out

    def stage_scan(self, blobs):
        """Host half of an ML observe (tables into a pinned staging slot), no kernel launched."""
        b = f64(blobs).reshape(-1, 4)
        check(self._lib.pk_stage_scan(self._h, dptr(b), b.shape[0]))

    def observe_staged(self, fresh=False):
        """Device half: upload + kernels for the scan staged last."""
        check(self._lib.pk_observe_staged(self._h, 1 if fresh else 0))

    def associate(self, blobs):
        b = f64(blobs).reshape(-1, 4)
        out = np.zeros((self.P, b.shape[0]), dtype=np.int32)
        check(self._lib.pk_associate(self._h, dptr(b), b.shape[0], iptr(out)))
        return out

    def resample(self, u, domain=PK_WEIGHTS_LINEAR, return_ancestors=False):
        out = np.empty(self.P, dtype=np.int64) if return_ancestors else None
        check(self._lib.pk_resample(self._h, float(u), int(domain), lptr(out)))
        return out

    def summary(self):
        out = np.empty(3, dtype=np.float64)
        check(self._lib.pk_summary(self._h, dptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def pose_sums(self):
        out = np.empty(4, dtype=np.float64)
        check(self._lib.pk_pose_sums(self._h, dptr(out)))
        return out

    def map_moments(self, weighting=PK_MAP_UNIFORM, gmax=None):
        """This handle's per-landmark moments over its particles (pk_map_moments) as ``mapsum.Moments``: what the shards of a
        filter combine.  gmax: the whole filter's maximum log-weight for PK_MAP_WEIGHTED (None: this handle's own)."""
        L = self.L
        wsum, mean, m2 = np.empty(2), np.empty((L, 5)), np.empty((L, 15))
        within, counts = np.empty((L, 9)), np.empty(L)
        check(self._lib.pk_map_moments(self._h, int(weighting), float("nan") if gmax is None else float(gmax), dptr(wsum), dptr(mean),
                                       dptr(m2), dptr(within), dptr(counts)))
        return mapsum.Moments(wsum, mean, m2, within, counts)

    def map_summary(self, weighting=PK_MAP_UNIFORM):
        """The map estimate of this filter (pk_map_summary) as ``mapsum.MapSummary``: per landmark the mean over the particles,
        the averaged EKF covariance, the covariance between the particles, the average update count; and n_eff."""
        L = self.L
        mean, within, between = np.empty((L, 5)), np.empty((L, 5, 5)), np.empty((L, 5, 5))
        count, n_eff = np.empty(L), np.empty(1)
        check(self._lib.pk_map_summary(self._h, int(weighting), dptr(mean), dptr(within), dptr(between), dptr(count), dptr(n_eff)))
        return mapsum.MapSummary(mean, within, between, count, n_eff[0])

    def map_match_moments(self, ref_means, radius, colour_radius, weighting=PK_MAP_UNIFORM, gmax=None, matches=False):
        """The moments of the particles' spare slots matched against the reference features ``ref_means`` (n, 5)
        (pk_map_match_moments) as ``mapsum.MatchedMoments``; matches=True: also the match table (P, n) int32, the spare slot of
        every particle matched to every feature or -1.  A slot matches a feature inside both radii, the smallest normalised
        distance wins; the matches are taken per feature, NOT one-to-one: keep ``radius`` below half the smallest landmark
        separation.  gmax as for map_moments."""
        ref = f64(ref_means).reshape(-1, 5)
        n = ref.shape[0]
        wsum, support, mean, m2 = np.empty(2), np.empty((n, 3)), np.empty((n, 5)), np.empty((n, 15))
        within, counts = np.empty((n, 9)), np.empty(n)
        table = np.empty((self.P, n), dtype=np.int32) if matches else None
        check(self._lib.pk_map_match_moments(self._h, int(weighting), float("nan") if gmax is None else float(gmax), dptr(ref), n,
                                             float(radius), float(colour_radius), dptr(wsum), dptr(support), dptr(mean), dptr(m2),
                                             dptr(within), dptr(counts), iptr(table)))
        return mapsum.MatchedMoments(wsum, support, mean, m2, within, counts, table)

    def map_discovered(self, radius, colour_radius, weighting=PK_MAP_UNIFORM, reference=None):
        """The estimate of the discovered landmarks (pk_map_discovered) as ``mapsum.DiscoveredMap``: the spare slots in use of
        the reference particle (None: the most likely one, ``best_particle()``'s) matched in every particle, and per feature the
        mean, the covariances and the share of the population that holds it.  The matches are NOT one-to-one: keep ``radius``
        below half the smallest landmark separation."""
        L0, S, _ = self.grow_shape()
        who, n = C.c_int64(-1), C.c_int32(0)
        ids, ref_counts = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
        mean, within, between = np.empty((S, 5)), np.empty((S, 5, 5)), np.empty((S, 5, 5))
        count, support, potential, n_eff, n_eff_all = np.empty(S), np.empty(S), np.empty(S), np.empty(S), np.empty(1)
        check(self._lib.pk_map_discovered(self._h, int(weighting), -1 if reference is None else int(reference), float(radius),
                                          float(colour_radius), C.byref(who), C.byref(n), iptr(ids), iptr(ref_counts), dptr(mean),
                                          dptr(within), dptr(between), dptr(count), dptr(support), dptr(potential), dptr(n_eff),
                                          dptr(n_eff_all)))
        k = int(n.value)
        return mapsum.DiscoveredMap(mean[:k], within[:k], between[:k], count[:k], support[:k], potential[:k], n_eff[:k], n_eff_all[0],
                                    reference_particle=int(who.value), ids=ids[:k], slots=L0 + np.arange(k), ref_counts=ref_counts[:k])

    # -- the path estimate (pk_path_*): rows 0 .. held - 1 are the recorded steps, oldest first; row held is the current generation
    def path_enable(self, capacity):
        """A ring of the last ``capacity`` resampled generations (0: off, memory released); every resample records a row."""
        check(self._lib.pk_path_enable(self._h, int(capacity)))

    def path_shape(self):
        """(capacity, rows held, rows ever recorded)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int64()
        check(self._lib.pk_path_shape(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def path_download(self, t0=0, t1=None):
        """(poses (n, P, 3), ancestors (n, P) int32) of the held rows [t0, t1)."""
        t1 = self.path_shape()[1] if t1 is None else int(t1)
        n = max(t1 - int(t0), 0)
        poses, anc = np.empty((n, self.P, 3), dtype=np.float64), np.empty((n, self.P), dtype=np.int32)
        check(self._lib.pk_path_download(self._h, int(t0), t1, dptr(poses), iptr(anc)))
        return poses, anc

    def path_upload(self, poses, ancestors, recorded=None):
        """Replaces the ring by n rows (snapshot restore, tests); recorded: the counter to go on from (default n)."""
        a = np.ascontiguousarray(ancestors, dtype=np.int32).reshape(-1, self.P)
        n = a.shape[0]
        p = f64(poses, (n, self.P, 3))
        check(self._lib.pk_path_upload(self._h, n, n if recorded is None else int(recorded), dptr(p), iptr(a)))

    def path_trace(self, particles):
        """The paths of the listed current particles, (len, held + 1, 3): bit for bit what was recorded."""
        idx = np.ascontiguousarray(particles, dtype=np.int64).reshape(-1)
        out = np.empty((idx.size, self.path_shape()[1] + 1, 3), dtype=np.float64)
        check(self._lib.pk_path_trace(self._h, lptr(idx), idx.size, dptr(out)))
        return out

    def path_summary(self):
        """The smoothed path over the P lineages as ``path.PathSummary``: per row mean (x, y, circular mean heading), spread
        (var x, cov xy, var y, mean resultant length) and the number of distinct ancestors the population still has there."""
        _, held, recorded = self.path_shape()
        mean, spread, surv = np.empty((held + 1, 3)), np.empty((held + 1, 4)), np.empty(held + 1, dtype=np.int64)
        check(self._lib.pk_path_summary(self._h, dptr(mean), dptr(spread), lptr(surv)))
        return path.PathSummary(mean, spread, surv, recorded - held)

    def path_summary_weighted(self, domain=PK_WEIGHTS_LINEAR):
        """The smoothed path by the weights of the current particles (pk_path_summary_weighted) as ``path.WeightedPathSummary``:
        path_summary's mean and spread per row, and the n_eff of the current weights."""
        _, held, recorded = self.path_shape()
        mean, spread, n_eff = np.empty((held + 1, 3)), np.empty((held + 1, 4)), np.empty(1)
        check(self._lib.pk_path_summary_weighted(self._h, int(domain), dptr(mean), dptr(spread), dptr(n_eff)))
        return path.WeightedPathSummary(mean, spread, n_eff[0], recorded - held)

    # -- the trunk (pk_path_trunk_*): the rows the ring has given up, 13 doubles each, at global steps first_step ..
    def path_trunk_enable(self, batch):
        """Settle the oldest ``batch`` rows into the trunk whenever a record fills the ring (0: off, memory released)."""
        check(self._lib.pk_path_trunk_enable(self._h, int(batch)))

    def path_settle(self, rows, weighting=PK_PATH_UNIFORM):
        """Settle the oldest ``rows`` held rows now, by PK_WEIGHTS_LINEAR / PK_WEIGHTS_LOG / PK_PATH_UNIFORM."""
        check(self._lib.pk_path_settle(self._h, int(rows), int(weighting)))

    def path_trunk_shape(self):
        """(batch, first_step, length)."""
        a, b, c = C.c_int32(), C.c_int64(), C.c_int64()
        check(self._lib.pk_path_trunk_shape(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def _trunk_range(self, s0, s1):
        _, first, n = self.path_trunk_shape()
        return (first if s0 is None else int(s0)), (first + n if s1 is None else int(s1))

    def path_trunk_download(self, s0=None, s1=None):
        """The raw trunk rows of global steps [s0, s1) (default: all), (n, 13): what a snapshot carries."""
        s0, s1 = self._trunk_range(s0, s1)
        rows = np.empty((max(s1 - s0, 0), path.TRUNK_RES), dtype=np.float64)
        check(self._lib.pk_path_trunk_download(self._h, s0, s1, dptr(rows)))
        return rows

    def path_trunk_upload(self, rows, first_step=0):
        """Replaces the trunk by ``rows`` (n, 13) from ``first_step`` on; only while the ring holds no rows."""
        r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, path.TRUNK_RES)
        check(self._lib.pk_path_trunk_upload(self._h, int(first_step), r.shape[0], dptr(r)))

    def path_trunk_summary(self, s0=None, s1=None):
        """(mean (n, 3), spread (n, 4), ancestors (n, 2) int64 = lo, hi) of the trunk's steps [s0, s1) (default: all)."""
        s0, s1 = self._trunk_range(s0, s1)
        n = max(s1 - s0, 0)
        mean, spread, anc = np.empty((n, 3)), np.empty((n, 4)), np.empty((n, 2), dtype=np.int64)
        check(self._lib.pk_path_trunk_summary(self._h, s0, s1, dptr(mean), dptr(spread), lptr(anc)))
        return mean, spread, anc

    def best_particle(self):
        """(index, log-weight) of the particle with the largest log-weight: the lowest index among equals, NaN never."""
        i, v = C.c_int64(), C.c_double()
        check(self._lib.pk_best_particle(self._h, C.byref(i), C.byref(v)))
        return int(i.value), float(v.value)

    def step(self, v, w, dt, blobs, u, z=None, seed=0, draw=0, ids=None, domain=PK_WEIGHTS_LINEAR):
        b = f64(blobs).reshape(-1, 4)
        B = b.shape[0]
        zz = f64(z, (self.P, 3)) if z is not None else None
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(B) if ids is not None else None
        check(self._lib.pk_step(self._h, float(v), float(w), float(dt), dptr(zz), int(seed), int(draw), dptr(b), B,
                                iptr(i), float(u), int(domain)))

    def step_odom(self, delta, alphas, blobs, u, threshold=None, z=None, seed=0, draw=0, ids=None, domain=PK_WEIGHTS_LINEAR):
        """step with motion_odom for its motion; threshold None: step's reset and resample, else step_adaptive's gate."""
        d, a = f64(delta, (3,)), f64(alphas, (4,))
        b = f64(blobs).reshape(-1, 4)
        B = b.shape[0]
        zz = f64(z, (self.P, 3)) if z is not None else None
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(B) if ids is not None else None
        check(self._lib.pk_step_odom(self._h, dptr(d), dptr(a), dptr(zz), int(seed), int(draw), dptr(b), B, iptr(i), float(u),
                                     int(domain), float("nan") if threshold is None else float(threshold)))

    # -- adaptive resampling (pk_resample_adaptive ...): the device decides, the host asks when it wants to know
    def resample_adaptive(self, u, threshold, domain=PK_WEIGHTS_LINEAR, return_ancestors=False):
        """Resamples iff n_eff < threshold * P (decided on the device); else the particles stay and the ancestors are arange(P)."""
        out = np.empty(self.P, dtype=np.int64) if return_ancestors else None
        check(self._lib.pk_resample_adaptive(self._h, float(u), int(domain), float(threshold), lptr(out)))
        return out

    def step_adaptive(self, v, w, dt, blobs, u, threshold, z=None, seed=0, draw=0, ids=None, domain=PK_WEIGHTS_LINEAR):
        """motion, observe with the weights carried over, resample_adaptive: no host synchronisation."""
        b = f64(blobs).reshape(-1, 4)
        B = b.shape[0]
        zz = f64(z, (self.P, 3)) if z is not None else None
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(B) if ids is not None else None
        check(self._lib.pk_step_adaptive(self._h, float(v), float(w), float(dt), dptr(zz), int(seed), int(draw), dptr(b), B,
                                         iptr(i), float(u), int(domain), float(threshold)))

    def resample_stats(self):
        """What the last gated call decided and the counters so far, as ``adaptive.ResampleStats``."""
        out, flag, counts = np.empty(4, dtype=np.float64), C.c_int32(), np.empty(2, dtype=np.int64)
        check(self._lib.pk_resample_stats(self._h, dptr(out), C.byref(flag), lptr(counts)))
        return adaptive.ResampleStats(out[0], out[1], out[2], out[3], flag.value != 0, counts[0], counts[1])

    def weight_sums(self, domain=PK_WEIGHTS_LINEAR, gmax=None):
        """(S1, S2) of this handle's current weights, summed as the gate sums them: what the shards of a filter would add.
        gmax: the whole filter's maximum log-weight for PK_WEIGHTS_LOG (None: this handle's own)."""
        out = np.empty(2, dtype=np.float64)
        check(self._lib.pk_weight_sums(self._h, int(domain), float("nan") if gmax is None else float(gmax), dptr(out)))
        return float(out[0]), float(out[1])

    def n_eff(self, domain=PK_WEIGHTS_LINEAR):
        """The effective sample size of the current weights: the gate's expression on weight_sums()."""
        s1, s2 = self.weight_sums(domain)
        with np.errstate(invalid="ignore", divide="ignore"):  # (every weight zero: NaN, as on the device)
            return float(np.float64(s1) / np.float64(s2) * np.float64(s1))

    def summary_weighted(self, domain=PK_WEIGHTS_LINEAR):
        """The pose estimate by the weights (pk_summary_weighted) as ``adaptive.PoseSummary``."""
        mean, spread, n_eff = np.empty(3), np.empty(4), np.empty(1)
        check(self._lib.pk_summary_weighted(self._h, int(domain), dptr(mean), dptr(spread), dptr(n_eff)))
        return adaptive.PoseSummary(mean, spread, n_eff[0])

    # -- sharded resample (see sharded.py) ---------------------------------------
    def set_shard(self, global_offset):
        check(self._lib.pk_set_shard(self._h, int(global_offset)))

    def shard_max_logw(self):
        v = C.c_double()
        check(self._lib.pk_shard_max_logw(self._h, C.byref(v)))
        return float(v.value)

    def shard_num_blocks(self):
        return int(self._lib.pk_shard_num_blocks(self._h))

    def shard_block_totals(self, gmax, domain):
        out = np.empty(self.shard_num_blocks(), dtype=np.float64)
        check(self._lib.pk_shard_block_totals(self._h, float(gmax), int(domain), dptr(out)))
        return out

    def shard_offspring(self, global_totals, first_block, global_particles, u, last_shard):
        t = f64(global_totals)
        out = np.empty(self.P + 1, dtype=np.int64)
        check(self._lib.pk_shard_offspring(self._h, dptr(t), t.size, int(first_block), int(global_particles), float(u),
                                           1 if last_shard else 0, lptr(out)))
        return out

    def shard_max_logw_dev(self, out_ptr):
        check(self._lib.pk_shard_max_logw_dev(self._h, C.c_void_p(out_ptr)))

    def shard_block_totals_dev(self, gmax_ptr, domain, totals_ptr):
        check(self._lib.pk_shard_block_totals_dev(self._h, C.c_void_p(gmax_ptr), int(domain), C.c_void_p(totals_ptr)))

    def shard_plan_dev(self, gtotals_ptr, n_blocks, first_block, global_particles, u, last_shard, world, ranges_ptr):
        check(self._lib.pk_shard_plan_dev(self._h, C.c_void_p(gtotals_ptr), int(n_blocks), int(first_block),
                                          int(global_particles), float(u), 1 if last_shard else 0, int(world),
                                          C.c_void_p(ranges_ptr)))

    def shard_logw_dev(self, out_ptr):
        check(self._lib.pk_shard_logw_dev(self._h, C.c_void_p(out_ptr)))

    def shard_plan_global_dev(self, glogw_ptr, global_particles, gmax_ptr, domain, u, last_shard, world, ranges_ptr):
        check(self._lib.pk_shard_plan_global_dev(self._h, C.c_void_p(glogw_ptr), int(global_particles), C.c_void_p(gmax_ptr),
                                                 int(domain), float(u), 1 if last_shard else 0, int(world), C.c_void_p(ranges_ptr)))

    def shard_download_offspring(self):
        out = np.empty(self.P + 1, dtype=np.int64)
        check(self._lib.pk_shard_download_offspring(self._h, lptr(out)))
        return out

    def shard_pack_dev(self, ranges, world, rank, buf_ptr):
        r = np.ascontiguousarray(ranges, dtype=np.int64)
        check(self._lib.pk_shard_pack_dev(self._h, lptr(r), int(world), int(rank), C.c_void_p(buf_ptr)))

    def shard_pack_slots_dev(self, j0, j1, slot_lo, slot_hi, buf_ptr):
        check(self._lib.pk_shard_pack_slots_dev(self._h, int(j0), int(j1), int(slot_lo), int(slot_hi), C.c_void_p(buf_ptr)))

    def shard_adopt_dev(self, rank, recv_ptr, n_received):
        check(self._lib.pk_shard_adopt_dev(self._h, int(rank), C.c_void_p(recv_ptr), int(n_received)))

    # -- the split step (the exchange overlapped with the work on the particles that stay) --
    def shard_local_span_dev(self, out_ptr):
        check(self._lib.pk_shard_local_span_dev(self._h, C.c_void_p(out_ptr)))

    def shard_adopt_local_dev(self, rank):
        check(self._lib.pk_shard_adopt_local_dev(self._h, int(rank)))

    def shard_adopt_remote_dev(self, rank, recv_ptr, n_received):
        check(self._lib.pk_shard_adopt_remote_dev(self._h, int(rank), C.c_void_p(recv_ptr), int(n_received)))

    # -- balanced placement (minimum migration) --
    def shard_state_dev(self, out_ptr):
        check(self._lib.pk_shard_state_dev(self._h, C.c_void_p(out_ptr)))

    def shard_plan_balanced_dev(self, gstate_ptr, global_particles, gmax_ptr, domain, u, world, rank, table_ptr):
        check(self._lib.pk_shard_plan_balanced_dev(self._h, C.c_void_p(gstate_ptr), int(global_particles), C.c_void_p(gmax_ptr),
                                                   int(domain), float(u), int(world), int(rank), C.c_void_p(table_ptr)))

    def shard_pack_balanced_dev(self, table, world, rank, buf_ptr):
        t = np.ascontiguousarray(table, dtype=np.int64)
        check(self._lib.pk_shard_pack_balanced_dev(self._h, lptr(t), int(world), int(rank), C.c_void_p(buf_ptr)))

    def shard_adopt_balanced_dev(self, table, world, rank, recv_ptr, n_received, mode):
        t = np.ascontiguousarray(table, dtype=np.int64)
        check(self._lib.pk_shard_adopt_balanced_dev(self._h, lptr(t), int(world), int(rank), C.c_void_p(recv_ptr), int(n_received),
                                                    int(mode)))

    def shard_pack_balanced_loop_dev(self, keep, a0, a1, buf_ptr):
        check(self._lib.pk_shard_pack_balanced_loop_dev(self._h, int(keep), int(a0), int(a1), C.c_void_p(buf_ptr)))

    def download_logical(self):
        out = np.empty(self.P, dtype=np.int64)
        check(self._lib.pk_shard_download_logical(self._h, lptr(out)))
        return out

    def upload_logical(self, logical):
        a = np.ascontiguousarray(logical, dtype=np.int64).reshape(self.P)
        check(self._lib.pk_shard_upload_logical(self._h, lptr(a)))

    def shard_download_balanced_plan(self):
        """(rel int64[P + 1], Hl int64[P], alive int32[n_alive]) of the last balanced plan (tests)."""
        rel, Hl, alive = np.empty(self.P + 1, dtype=np.int64), np.empty(self.P, dtype=np.int64), np.empty(self.P, dtype=np.int32)
        check(self._lib.pk_shard_download_balanced_plan(self._h, lptr(rel), lptr(Hl), iptr(alive)))
        return rel, Hl, alive[alive >= 0]

    def reset_placement(self):
        check(self._lib.pk_shard_reset_placement(self._h))

    def shard_download_balanced_offspring(self, global_particles):
        out = np.empty(int(global_particles) + 1, dtype=np.int64)
        check(self._lib.pk_shard_download_balanced_offspring(self._h, int(global_particles), lptr(out)))
        return out

    def shard_balanced_errors(self):
        out = np.zeros(1, dtype=np.int64)
        check(self._lib.pk_shard_balanced_errors(self._h, lptr(out)))
        return int(out[0])

    def motion_range(self, v, w, dt, seed, draw, p0, p1):
        check(self._lib.pk_motion_range(self._h, float(v), float(w), float(dt), int(seed), int(draw), int(p0), int(p1)))

    def motion_odom_range(self, delta, alphas, seed, draw, p0, p1):
        d, a = f64(delta, (3,)), f64(alphas, (4,))
        check(self._lib.pk_motion_odom_range(self._h, dptr(d), dptr(a), int(seed), int(draw), int(p0), int(p1)))

    def staged_takes_regs(self):
        return bool(self._lib.pk_staged_takes_regs(self._h))

    def observe_staged_range(self, fresh, p0, p1, first, last):
        check(self._lib.pk_observe_staged_range(self._h, 1 if fresh else 0, int(p0), int(p1), 1 if first else 0, 1 if last else 0))

    ROUTES = {0: "none", 1: "known_ids", 2: "ml_general", 3: "ml_handoff", 4: "ml_sweep", 5: "ml_fused", 6: "ml_regs", 8: "dense", 9: "ml_pub_big"}

    def observe_route(self):
        """Kernels the last observe / step used for association + EKF update (pk_observe_route)."""
        return self.ROUTES[int(self._lib.pk_observe_route(self._h))]

    def observe_flagged(self):
        """(particles the last ML observe handed to the general kernels, candidate-list overflows) -- pk_observe_flagged."""
        a, b = C.c_int64(), C.c_int64()
        check(self._lib.pk_observe_flagged(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def observe_pub_stats(self):
        """The last scan's publish table (pk_observe_pub_stats): dict of entries, contested blobs, landmarks of the reference
        particle with several blobs inside their gates, longest candidate list, entry capacity, instance (0 none, 1 one
        workgroup per CU, 2 and 3 k_step_pub_duo with "pub_duo" = 1 and 2)."""
        a = np.zeros(6, dtype=np.int64)
        check(self._lib.pk_observe_pub_stats(self._h, lptr(a)))
        return dict(zip(("entries", "contested_blobs", "multi_landmarks", "longest_list", "entry_capacity", "instance"), (int(v) for v in a)))

    def observe_lean_stats(self):
        """The last scan's lean groups (pk_observe_lean_stats): dict of marked (groups in use that the scan marked lean), in_use,
        fallbacks (pairs of lean groups that took the usual body after all)."""
        a = np.zeros(3, dtype=np.int64)
        check(self._lib.pk_observe_lean_stats(self._h, lptr(a)))
        return dict(zip(("marked", "in_use", "fallbacks"), (int(v) for v in a)))

    def colour_table_stats(self):
        """The colour table (pk_colour_table_stats): dict of engaged (the last observe ran in the mode and nothing has ended it),
        depth, scans (taken in the mode), materialisations (whole-buffer write-backs of the slots' colour rows)."""
        a = np.zeros(4, dtype=np.int64)
        check(self._lib.pk_colour_table_stats(self._h, lptr(a)))
        return dict(zip(("engaged", "depth", "scans", "materialisations"), (int(v) for v in a)))

    # ---- new landmarks on the device (pk_grow_enable) ----
    def grow_enable(self, preset_landmarks, reading_capacity=64, pair_threshold=30.0):
        check(self._lib.pk_grow_enable(self._h, int(preset_landmarks), int(reading_capacity), float(pair_threshold)))

    def grow_shape(self):
        """(preset landmarks, spare slots, reading capacity); zeros while the bookkeeping is off."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._lib.pk_grow_shape(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def grow_init(self, mode, min_parallax=0.0):
        """How the bookkeeping places a new feature from the next scan on (pk_grow_init): "reference" (any crossing, identity
        position covariance) or "triangulated" (crossings at ``min_parallax`` radians or more, the triangulation's own covariance)
        -- or PK_GROW_INIT_*."""
        if isinstance(mode, str):
            if mode not in LANDMARK_INITS:
                raise ValueError("grow_init: %r is neither %s" % (mode, " nor ".join(repr(k) for k in LANDMARK_INITS)))
            mode = LANDMARK_INITS[mode]
        check(self._lib.pk_grow_init(self._h, int(mode), float(min_parallax)))

    def grow_init_mode(self):
        """(mode's name, min_parallax) as pk_grow_init last took them; ("reference", 0.0) on a filter that never asked."""
        m, a = C.c_int32(), C.c_double()
        check(self._lib.pk_grow_init_mode(self._h, C.byref(m), C.byref(a)))
        return {v: k for k, v in LANDMARK_INITS.items()}[int(m.value)], float(a.value)

    def grow_ranges(self, on=True):
        """Ranged scans on a growing map (pk_grow_ranges): on, the calls that take blobs consume the ranges scan_ranges armed, and an
        unmatched blob with a range becomes a potential feature at once, at the measured point with its covariance; a blob without
        one goes through grow_init's rule.  Off (the default), such a scan is refused as ever.  ``on`` is 0 or 1 (or a bool)."""
        check(self._lib.pk_grow_ranges(self._h, int(on)))

    def grow_ranges_state(self):
        """Whether a growing map takes ranged scans: pk_grow_ranges_state."""
        on = C.c_int32()
        check(self._lib.pk_grow_ranges_state(self._h, C.byref(on)))
        return bool(on.value)

    def grow_download(self, p0=0, p1=None, counters=True, readings=True, slot_ids=True):
        """(counters (n, 4) int32: readings stored / spare slots in use / next_id / readings dropped,
        readings (n, R, 8): id, x, y, heading, bearing, r, g, b, slot_ids (n, S) int32); None for what was not asked for."""
        p1 = self.P if p1 is None else p1
        _, S, R = self.grow_shape()
        n = p1 - p0
        c = np.empty((n, 4), dtype=np.int32) if counters else None
        r = np.empty((n, R, 8), dtype=np.float64) if readings else None
        s = np.empty((n, S), dtype=np.int32) if slot_ids else None
        check(self._lib.pk_grow_download(self._h, int(p0), int(p1), iptr(c), dptr(r), iptr(s)))
        return c, r, s

    def grow_upload(self, p0, p1, counters=None, readings=None, slot_ids=None):
        _, S, R = self.grow_shape()
        n = p1 - p0
        c = None if counters is None else np.ascontiguousarray(counters, dtype=np.int32).reshape(n, 4)
        r = None if readings is None else f64(readings, (n, R, 8))
        s = None if slot_ids is None else np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(n, S)
        check(self._lib.pk_grow_upload(self._h, int(p0), int(p1), iptr(c), dptr(r), iptr(s)))

    def grow_retire(self, reading_max_age=0, potential_max_idle=0):
        """Retire readings older than ``reading_max_age`` scans and potential features unmatched for ``potential_max_idle`` scans,
        behind every scan's bookkeeping (0: never; both 0: off, and the clocks' memory goes back)."""
        check(self._lib.pk_grow_retire(self._h, int(reading_max_age), int(potential_max_idle)))

    def grow_clocks_download(self, p0=0, p1=None):
        """(counters (n, 4) int32: readings covered / slots covered / readings retired / features retired, reading_scan (n, R) uint32,
        slot_seen (n, S) int32, slot_idle (n, S) int32, scan_now) while retirement is on."""
        p1 = self.P if p1 is None else p1
        _, S, R = self.grow_shape()
        n = p1 - p0
        c, sc = np.empty((n, 4), dtype=np.int32), np.empty((n, R), dtype=np.uint32)
        se, si = np.empty((n, S), dtype=np.int32), np.empty((n, S), dtype=np.int32)
        now = C.c_uint32(0)
        check(self._lib.pk_grow_clocks_download(self._h, int(p0), int(p1), iptr(c), sc.ctypes.data_as(_up), iptr(se), iptr(si), C.byref(now)))
        return c, sc, se, si, int(now.value)

    def grow_clocks_upload(self, p0, p1, counters=None, reading_scan=None, slot_seen=None, slot_idle=None, scan_now=None):
        _, S, R = self.grow_shape()
        n = p1 - p0
        c = None if counters is None else np.ascontiguousarray(counters, dtype=np.int32).reshape(n, 4)
        sc = None if reading_scan is None else np.ascontiguousarray(reading_scan, dtype=np.uint32).reshape(n, R)
        se = None if slot_seen is None else np.ascontiguousarray(slot_seen, dtype=np.int32).reshape(n, S)
        si = None if slot_idle is None else np.ascontiguousarray(slot_idle, dtype=np.int32).reshape(n, S)
        now = None if scan_now is None else C.byref(C.c_uint32(int(scan_now) & 0xFFFFFFFF))
        check(self._lib.pk_grow_clocks_upload(self._h, int(p0), int(p1), iptr(c), None if sc is None else sc.ctypes.data_as(_up), iptr(se),
                                              iptr(si), now))

    def grow_view(self, half_fov, range_min=0.0, range_max=float("inf"), confirmed_max_misses=0):
        """The sensor's field for the retirement pass (pk_grow_view): an unmatched spare slot ages only while its position mean lies
        within ``half_fov`` of the particle's heading and between the two ranges, and a promoted feature goes after
        ``confirmed_max_misses`` such misses (0: never).  ``half_fov=0``: off."""
        check(self._lib.pk_grow_view(self._h, float(half_fov), float(range_min), float(range_max), int(confirmed_max_misses)))

    def grow_view_state(self):
        """(on, (half_fov, range_min, range_max), confirmed_max_misses) -- pk_grow_view_state."""
        on, c, v = C.c_int32(), C.c_int32(), np.zeros(3, dtype=np.float64)
        check(self._lib.pk_grow_view_state(self._h, C.byref(on), dptr(v), C.byref(c)))
        return bool(on.value), (float(v[0]), float(v[1]), float(v[2])), int(c.value)

    def grow_view_stats(self):
        """int64[4] (pk_grow_view_stats; synchronises): of the last pass, the known slots that did not change and the ones of those
        in view; potential and confirmed features retired since the view was switched on -- summed over the particles."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.pk_grow_view_stats(self._h, out.ctypes.data_as(_lp)))
        return out

    def observe_retry_rows(self):
        """(second-chance rows the last scan wanted, rows the next scan will find) -- pk_observe_retry_rows."""
        a, b = C.c_int64(), C.c_int64()
        check(self._lib.pk_observe_retry_rows(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def observe_published(self):
        """True when k_step_pub (static publish / subscribe settling) worked on the last register-route scan."""
        v = C.c_int32()
        check(self._lib.pk_observe_published(self._h, C.byref(v)))
        return bool(v.value)

    def observe_flags(self):
        """Per particle: 0 = settled by the one-pass kernel, 2 = second-chance route, 1 = general kernels (pk_observe_flags)."""
        out = np.zeros(self.P, dtype=np.uint8)
        check(self._lib.pk_observe_flags(self._h, out.ctypes.data_as(_bp)))
        return out

    def download_sources(self):
        """Map slot each particle's landmarks currently live in (pk_download_sources)."""
        out = np.empty(self.P, dtype=np.int32)
        check(self._lib.pk_download_sources(self._h, iptr(out)))
        return out

    def particle_bytes(self):
        return int(self._lib.pk_particle_bytes(self._h))

    def pack_particles(self, local_idx, dev_ptr):
        idx = np.ascontiguousarray(local_idx, dtype=np.int64)
        check(self._lib.pk_pack_particles(self._h, lptr(idx), idx.size, C.c_void_p(dev_ptr)))

    def adopt_particles(self, src, dev_ptr, n_received):
        s_ = np.ascontiguousarray(src, dtype=np.int64).reshape(self.P)
        check(self._lib.pk_adopt_particles(self._h, lptr(s_), C.c_void_p(dev_ptr), int(n_received)))

    # -- instrumentation -----------------------------------------------------
    def enable_timing(self, mask=True):
        """mask: True = every kernel slot, False/0 = off, int = bitmask over PK_T_NAMES."""
        m = -1 if mask is True else (0 if mask is False else int(mask))
        check(self._lib.pk_enable_timing(self._h, m))

    def reset_timings(self):
        check(self._lib.pk_reset_timings(self._h))

    def timings(self):
        ms = np.zeros(PK_T_COUNT, dtype=np.float64)
        n = np.zeros(PK_T_COUNT, dtype=np.int64)
        check(self._lib.pk_timings(self._h, dptr(ms), lptr(n)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(PK_T_NAMES)}

    def observe_bytes(self, num_blobs):
        a = C.c_int64()
        m = C.c_int64()
        check(self._lib.pk_observe_bytes(self._h, int(num_blobs), C.byref(a), C.byref(m)))
        return int(a.value), int(m.value)


def probe(pose, mean, cov, blob, Qt=None, device=0):
    """Evaluate every scalar function of the path on one (pose, landmark, blob) on the GPU."""
    lib = load()
    Qt = 0.1 * np.identity(4) if Qt is None else Qt
    out = np.empty(PK_PROBE_LEN, dtype=np.float64)
    check(lib.pk_probe(int(device), dptr(f64(pose, (3,))), dptr(f64(mean, (5,))), dptr(f64(cov, (25,))),
                       dptr(f64(blob, (4,))), dptr(f64(Qt, (16,))), dptr(out)))
    return dict(
        probability_of_match=out[0], prob_position_match=out[1], closest_point=out[2:4].copy(),
        prob_color_match=out[4], zhat=out[5:9].copy(), H0=out[9:11].copy(), Q=out[11:27].reshape(4, 4).copy(),
        K=out[27:47].reshape(5, 4).copy(), weight=out[47], new_mean=out[48:53].copy(),
        new_cov=out[53:78].reshape(5, 5).copy(), log_weight=out[78],
    )


def probe_math(op, array, device=0):
    """One float64 primitive of the kernels (PK_MATH_*) on the rows of ``array`` (n x arity; a flat array for arity 1) on the GPU
    (pk_probe_math): the n results, or (n, outputs).  PK_MATH_KEY returns (keys uint64[n], round trip float64[n])."""
    lib = load()
    arity, outputs = PK_MATH_SHAPES[int(op)]
    a = f64(array, (-1, arity))
    n = a.shape[0]
    out = np.empty((n, outputs), dtype=np.float64)
    check(lib.pk_probe_math(int(device), int(op), n, dptr(a), dptr(out)))
    if op == PK_MATH_KEY:
        return out[:, 0].copy().view(np.uint64), out[:, 1].copy()
    return out[:, 0].copy() if outputs == 1 else out


def probe_bearing(what, array, device=0):
    """The bearing model's primitives on the rows of ``array`` on the GPU (pk_probe_bearing): what 0 the match probabilities
    (n x 23 -> n x 5), 1 the update (n x 32 -> n x 17)."""
    lib = load()
    arity, outputs = PK_BEARING_SHAPES.get(int(what), (1, 1))
    a = f64(array, (-1, arity))
    out = np.empty((a.shape[0], outputs), dtype=np.float64)
    check(lib.pk_probe_bearing(int(device), int(what), a.shape[0], dptr(a), dptr(out)))
    return out


def probe_range(what, array, device=0):
    """The primitives of range-bearing blobs on the rows of ``array`` on the GPU (pk_probe_range): what 0 the match probabilities
    (n x 26 -> n x 5), 1 the update (n x 33 -> n x 16)."""
    lib = load()
    arity, outputs = PK_RANGE_SHAPES.get(int(what), (1, 1))
    a = f64(array, (-1, arity))
    out = np.empty((a.shape[0], outputs), dtype=np.float64)
    check(lib.pk_probe_range(int(device), int(what), a.shape[0], dptr(a), dptr(out)))
    return out


class HostRng(object):
    """Host reproduction of numpy's legacy normal stream / CPython's random() (pk_rng_*)."""

    def __init__(self, seed, kind="numpy"):
        self._lib = load()
        self._h = _h()
        fn = self._lib.pk_rng_create_numpy if kind == "numpy" else self._lib.pk_rng_create_python
        check(fn(int(seed) & 0xFFFFFFFF, C.byref(self._h)))

    def standard_normal(self, n):
        out = np.empty(int(n), dtype=np.float64)
        check(self._lib.pk_rng_standard_normal(self._h, int(n), dptr(out)))
        return out

    def random(self, n=None):
        out = np.empty(1 if n is None else int(n), dtype=np.float64)
        check(self._lib.pk_rng_random(self._h, out.size, dptr(out)))
        return float(out[0]) if n is None else out

    def __del__(self):
        try:
            if self._h.value:
                self._lib.pk_rng_destroy(self._h)
                self._h = _h()
        except Exception:
            pass

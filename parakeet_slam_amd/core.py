"""FastSLAM / FilterParticle / Feature: the reference's class surface over the HIP library.

This mirrors ``/root/reference/src/prkt_core_v2.py`` name for name (same constructor
arguments, attributes, method names, argument meaning and error behaviour) so that its
only caller, ``prkt_ros.py`` (left untouched), can ``from parakeet_slam_amd import
FastSLAM, Feature`` instead of ``from prkt_core_v2 import ...`` -- see INTEGRATION.md.

What is different on purpose:
  * all per-particle state lives in HBM behind one ``pk_filter`` handle; ``particles`` is
    a list-like of lazily materialised ``FilterParticle`` snapshots;
  * ``num_particles`` is a constructor keyword (the reference hard-codes 50, :41);
  * one lock serialises ``cam_cb`` / ``motion_update`` / ``summary`` (the reference races
    between the rospy callback thread and the main loop);
  * the particle update itself (motion sample, data association, EKF, weights, resample,
    summary) runs ONLY on the GPU.  There is no CPU fallback: without the shared library
    or without a HIP device, construction raises.
"""
from __future__ import annotations

import copy as _copy
import inspect as _inspect
import math
import random as _pyrandom
import threading

import numpy as np

from . import _lib, adaptive, mapsum, msgs
from . import odom as _odom
from . import path as _path
from .msgs import Blob, Odometry, Twist, heading_to_quaternion, quaternion_to_heading

NO_MATCH_WEIGHT = 0.1  # prkt_core_v2.py:851-857


def _default_Qt():
    # prkt_core_v2.py:50-53
    return np.array([[.1, 0, 0, 0], [0, .1, 0, 0], [0, 0, .1, 0], [0, 0, 0, .1]])


def _blob_row(blob):
    """matrix.blob_to_matrix (matrix.py:35-39)."""
    if isinstance(blob, (np.ndarray, list, tuple)):
        return np.asarray(blob, dtype=np.float64).reshape(4)
    return np.array([blob.bearing, blob.color.r, blob.color.g, blob.color.b], dtype=np.float64)


def _check_association(association, proposal, devices, who="FastSLAM"):
    """association: 'ml' (every blob takes its own most likely landmark) or 'unique' (pk_assoc_unique: at most one blob of a scan
    keeps each landmark of a particle) -- the latter on one GPU, under the plain step."""
    if association not in ("ml", "unique"):
        raise ValueError("%s(association=%r): 'ml' (default) or 'unique'" % (who, association))
    if association == "unique" and proposal == "measurement":
        raise ValueError("%s(association='unique', proposal='measurement'): the measurement-informed proposal settles its own "
                         "tentative ids inside its kernel and has no unique pass yet; the plain step (proposal='motion') takes it"
                         % who)
    if association == "unique" and devices is not None and len(list(devices)) > 1:
        raise ValueError("%s(devices=[...], association='unique'): unique association runs on one GPU -- the kernel works per "
                         "particle and would serve every shard, but the shards' filters are not told of the mode" % who)
    return association


def _check_proposal_grow(proposal_grow, proposal, new_landmarks, spare_landmarks, bookkeeping, devices, range_noise, proposal_ranges,
                         grow_ranges, who="FastSLAM"):
    """proposal_grow=True: the measurement-informed proposal on a growing map (pk_proposal_grow) -- it needs proposal='measurement',
    new_landmarks=True with spare slots, the device bookkeeping and one GPU; a range_noise then goes through the proposal AND the
    bookkeeping (proposal_ranges=True and grow_ranges=True together)."""
    if not proposal_grow:
        return False
    if proposal != "measurement":
        raise ValueError("%s(proposal_grow=True): the proposal on growing maps is a mode of proposal='measurement'" % who)
    if not new_landmarks or not int(spare_landmarks) > 0:
        raise ValueError("%s(proposal_grow=True): the proposal on growing maps needs a map that grows: new_landmarks=True and "
                         "spare_landmarks > 0" % who)
    if bookkeeping != "device":
        raise ValueError("%s(proposal_grow=True): the new-landmark bookkeeping follows the proposal step on the device "
                         "(bookkeeping='device'), not bookkeeping='host'" % who)
    if devices is not None and len(list(devices)) > 1:
        raise ValueError("%s(devices=[...], proposal_grow=True): the measurement-informed proposal runs on one GPU" % who)
    if range_noise is not None and not (proposal_ranges and grow_ranges):
        raise ValueError("%s(range_noise=..., proposal_grow=True): the ranges of a growing map under the proposal enter both the "
                         "proposal and the bookkeeping: proposal_ranges=True and grow_ranges=True together" % who)
    return True


def _check_range_noise(range_noise, measurement_model, proposal, new_landmarks, who="FastSLAM", proposal_ranges=False,
                       grow_ranges=False, proposal_grow=False):
    """range_noise=(sigma0, sigma1) of FastSLAM: None, or the two floats of a range's standard deviation sigma0 + sigma1 rho.
    proposal_ranges=True: ranges enter the measurement-informed proposal -- it needs both range_noise and proposal='measurement'.
    grow_ranges=True: ranges on a growing map -- it needs range_noise, new_landmarks=True and proposal='motion' (the spare slots and
    the device bookkeeping are checked by _check_grow_ranges); proposal='measurement' takes it with proposal_grow=True
    (_check_proposal_grow has held that to its own conditions)."""
    if grow_ranges and (range_noise is None or not new_landmarks or (proposal == "measurement" and not proposal_grow)):
        raise ValueError("%s(grow_ranges=True): ranges on a growing map need range_noise=(sigma0, sigma1), new_landmarks=True and "
                         "proposal='motion'" % who)
    if proposal_ranges and (range_noise is None or proposal != "measurement"):
        raise ValueError("%s(proposal_ranges=True): ranges in the proposal need range_noise=(sigma0, sigma1) and "
                         "proposal='measurement'" % who)
    if range_noise is None:
        return None
    try:
        s0, s1 = (float(v) for v in range_noise)
    except (TypeError, ValueError):
        raise ValueError("%s(range_noise=%r): None, or (sigma0, sigma1) -- a range's standard deviation is sigma0 + sigma1 * range"
                         % (who, range_noise))
    if not (math.isfinite(s0) and math.isfinite(s1)) or s0 < 0.0 or s1 < 0.0:
        raise ValueError("%s(range_noise=%r): sigma0 and sigma1 are finite and >= 0" % (who, range_noise))
    if s0 == 0.0 and s1 == 0.0:
        raise ValueError("%s(range_noise=%r): a range needs a variance > 0 -- sigma0 and sigma1 cannot both be 0" % (who, range_noise))
    if measurement_model != "bearing":
        raise ValueError("%s(range_noise=...): per-blob ranges are an option of measurement_model='bearing'; the reference model "
                         "has no range" % who)
    if proposal == "measurement" and not proposal_ranges:
        raise ValueError("%s(range_noise=..., proposal='measurement'): the measurement-informed proposal samples the pose from the "
                         "bearings alone; ranges go with proposal='motion', or enter the proposal with proposal_ranges=True" % who)
    if new_landmarks and not grow_ranges:
        raise ValueError("%s(range_noise=..., new_landmarks=True): a growing map still places a new landmark from two bearings; "
                         "ranges go with a preset map" % who)
    return s0, s1


def _check_grow_ranges(grow_ranges, spare_landmarks, bookkeeping, who="FastSLAM"):
    """grow_ranges=True beyond what _check_range_noise holds it to: the single-sighting rule is the device kernel's."""
    if grow_ranges and not (int(spare_landmarks) > 0 and bookkeeping == "device"):
        raise ValueError("%s(grow_ranges=True): a new landmark is placed from one ranged sighting by the device bookkeeping of a "
                         "growing map (spare_landmarks > 0, bookkeeping='device'), not by bookkeeping='host'" % who)
    return bool(grow_ranges)


def _check_view(view, confirmed_max_misses, reading_max_age, potential_max_idle, new_landmarks, spare_landmarks, bookkeeping, devices,
                who="FastSLAM"):
    """view=(half_fov, r_min, r_max) / confirmed_max_misses=C -> ((half_fov, r_min, r_max) or None, C): the sensor's field for the
    retirement pass (pk_grow_view), which needs that pass -- a threshold, device bookkeeping, one GPU."""
    C = int(confirmed_max_misses)
    if view is None:
        if C:
            raise ValueError("%s(confirmed_max_misses=%d): a promoted feature's misses are counted inside a field of view -- give "
                             "view=(half_fov, r_min, r_max) with it" % (who, C))
        return None, 0
    try:
        half_fov, r_min, r_max = (float(v) for v in view)
    except (TypeError, ValueError):
        raise ValueError("%s(view=%r): (half_fov, r_min, r_max) -- radians in (0, pi], 0 <= r_min < r_max (r_max may be inf)" % (who, view))
    if not (0.0 < half_fov <= math.pi and 0.0 <= r_min < float("inf") and r_max > r_min):
        raise ValueError("%s(view=%r): (half_fov, r_min, r_max) -- radians in (0, pi], 0 <= r_min < r_max (r_max may be inf)" % (who, view))
    if not 0 <= C <= 2 ** 30:
        raise ValueError("%s(confirmed_max_misses=%d): a number of scans in 0..2^30 (0: a promoted feature is never retired)" % (who, C))
    if devices is not None and len(list(devices)) > 1:
        raise ValueError("%s(devices=[...], view=...): readings and features are retired on one GPU only -- a particle's record "
                         "carries no clocks from one rank to another" % who)
    if not (new_landmarks and int(spare_landmarks) > 0 and bookkeeping == "device"):
        raise ValueError("%s(view=...): features are retired by the device bookkeeping of a growing map (new_landmarks=True, "
                         "spare_landmarks > 0, bookkeeping='device'), not by bookkeeping='host'" % who)
    if not (int(reading_max_age) or int(potential_max_idle)):
        raise ValueError("%s(view=...): the field of view belongs to the retirement pass -- give reading_max_age=... or "
                         "potential_max_idle=... (potential_max_idle=2**30 retires confirmed features only)" % who)
    return (half_fov, r_min, r_max), C


def _scan_with_ranges(observes, range_noise, who="FastSLAM"):
    """(observes for _blob_matrix, ranges or None): a (B, 5) array (bearing, r, g, b, range) is split -- and refused without
    range_noise --; with range_noise, message objects are asked for an optional ``range`` attribute (absent, None or NaN: none)."""
    if isinstance(observes, np.ndarray) and observes.ndim == 2 and observes.shape[1] == 5:
        if range_noise is None:
            raise ValueError("%s: a (B, 5) scan (bearing, r, g, b, range) needs range_noise=(sigma0, sigma1); this filter takes "
                             "(B, 4) scans" % who)
        return observes[:, :4], np.array(observes[:, 4], dtype=np.float64)
    if range_noise is None or (isinstance(observes, np.ndarray) and observes.ndim == 2):
        return observes, None
    observes = list(observes)
    ranges = np.array([float("nan") if getattr(b, "range", None) is None else float(b.range) for b in observes], dtype=np.float64)
    return observes, ranges


def _blob_matrix(observes):
    """The scan as a (B, 4) array of (bearing, r, g, b) -- blob_to_matrix (matrix.py:35-39) for every blob of
    ``ros_view.last_sensor_reading.observes`` (prkt_core_v2.py:82, :344).  Message objects are read in one flat pass (2 000 blobs:
    0.6 ms of attribute reads instead of 2 ms of one small array per blob); a caller that already holds the scan as a (B, 4)
    array may hand that over as ``observes`` and pays nothing."""
    if isinstance(observes, np.ndarray) and observes.ndim == 2 and observes.shape[1] == 4:
        return np.ascontiguousarray(observes, dtype=np.float64)
    observes = list(observes)
    try:
        flat = [v for b in observes for c in (b.color,) for v in (b.bearing, c.r, c.g, c.b)]
        return np.array(flat, dtype=np.float64).reshape(-1, 4)
    except AttributeError:  # rows given as sequences, or a mix
        return np.array([_blob_row(b) for b in observes], dtype=np.float64).reshape(-1, 4)


def _state_pose(state):
    return (float(state.pose.pose.position.x), float(state.pose.pose.position.y),
            float(quaternion_to_heading(state.pose.pose.orientation)))


def _make_state(x, y, h):
    st = Odometry()
    st.pose.pose.position.x = float(x)
    st.pose.pose.position.y = float(y)
    st.pose.pose.orientation = heading_to_quaternion(float(h))
    return st


# =============================================================================
class Feature(object):
    """prkt_core_v2.py:881-930.  A landmark EKF: mean (x, y, r, g, b), covar 5x5."""

    def __init__(self, mean=None, covar=None):
        self.__immutable__ = False
        if mean is None:
            mean = np.array([0, 0, 0, 0, 0])
        if covar is None:
            covar = np.identity(5, dtype=np.int64)
        self.mean = np.array(mean)
        self.covar = np.array(covar)
        self.identity = np.identity(self.covar.shape[0])
        self.update_count = 0

    # The two methods below are the reference's object-level API (:897-930) for a caller
    # that already holds K and H as matrices.  cam_cb never calls them: inside the filter
    # the same update runs fused in the HIP kernel k_observe.  They are two NumPy products,
    # exactly as matrix.py defines them, kept so scripts that poke a lone Feature still run.
    def update_mean(self, kalman_gain, measure, expected_measure):
        if self.__immutable__:
            return None
        delz = _blob_row(measure) - _blob_row(expected_measure)
        self.mean = self.mean + np.dot(kalman_gain, delz)
        self.update_count += 1

    def update_covar(self, kalman_gain, bigH):
        if self.__immutable__:
            return None
        adjust = np.subtract(self.identity, np.dot(kalman_gain, bigH))
        self.covar = np.dot(adjust, self.covar)
        self.update_count += 1


# =============================================================================
class _FeatureSet(dict):
    """feature_set of a particle that lives on the GPU: downloaded on first touch."""

    def __init__(self, loader):
        super().__init__()
        self._loader = loader

    def _load(self):
        if self._loader is not None:
            ld, self._loader = self._loader, None
            for k, v in ld().items():
                dict.__setitem__(self, k, v)

    def __getitem__(self, k):
        self._load()
        return dict.__getitem__(self, k)

    def __iter__(self):
        self._load()
        return dict.__iter__(self)

    def __len__(self):
        self._load()
        return dict.__len__(self)

    def __contains__(self, k):
        self._load()
        return dict.__contains__(self, k)

    def keys(self):
        self._load()
        return dict.keys(self)

    def values(self):
        self._load()
        return dict.values(self)

    def items(self):
        self._load()
        return dict.items(self)

    def get(self, k, default=None):
        self._load()
        return dict.get(self, k, default)

    def __deepcopy__(self, memo):
        self._load()
        out = {}
        for k, v in dict.items(self):
            out[k] = _copy.deepcopy(v, memo)
        return out


class FilterParticle(object):
    """prkt_core_v2.py:278-877.  A robot pose hypothesis with its own landmark map.

    A standalone instance is a host object; its scalar methods evaluate the device
    functions of the HIP path on the GPU through ``pk_probe`` / a one-particle filter.
    ``FastSLAM.particles[i]`` yields snapshots of the particles that live in HBM.
    """

    Qt = _default_Qt()
    _device = 0

    def __init__(self, state=None):
        if state is None:
            state = _make_state(0.0, 0.0, 0.0)
        self.state = state
        self.feature_set = {}
        self.potential_features = {}
        self.weight = 1
        self.hypothesis_set = {}
        self.next_id = 1

    # -- bookkeeping (:294-315) ----------------------------------------------
    def load_feature_list(self, features):
        for feature in features:
            self.feature_set[self.next_id] = feature
            self.next_id += 1

    def get_feature_by_id(self, id_):
        if id_ < 0:
            return self.potential_features[int(id_)]
        return self.feature_set[id_]

    # -- device evaluation helpers ---------------------------------------------
    def _probe(self, pose, mean, cov, blob, Qt=None):
        return _lib.probe(pose, np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64), blob,
                          self.Qt if Qt is None else Qt, device=self._device)

    def _one_particle_filter(self, state):
        if len(self.potential_features):
            raise NotImplementedError(
                "potential (negative-id) features are outside the device path: the reference never "
                "creates one (SURVEY.md section 2, row 1b)")
        ids = sorted(self.feature_set.keys())
        f = _lib.DeviceFilter(1, len(ids), device=self._device)
        if ids:
            means = np.array([np.asarray(self.feature_set[i].mean, dtype=np.float64) for i in ids])
            covs = np.array([np.asarray(self.feature_set[i].covar, dtype=np.float64) for i in ids])
            imm = np.array([bool(self.feature_set[i].__immutable__) for i in ids], dtype=np.uint8)
            f.upload_map(means, covs.reshape(len(ids), 25), imm)
        x, y, h = _state_pose(state)
        f.upload_poses(np.array([[x, y, h, 1.0]]))
        return f, ids

    # -- a3: association (:317-381) ----------------------------------------------
    def match_features_to_scan(self, scan):
        blobs = list(scan.observes)
        if not blobs:
            return []
        f, ids = self._one_particle_filter(self.state)
        try:
            got = f.associate(np.array([_blob_row(b) for b in blobs]))[0]
        finally:
            f.close()
        return [((ids[g - 1] if g > 0 else 0), b) for g, b in zip(got, blobs)]

    def match_one(self, state, blob):
        f, ids = self._one_particle_filter(state)
        try:
            g = int(f.associate(_blob_row(blob)[None, :])[0, 0])
        finally:
            f.close()
        return ids[g - 1] if g > 0 else 0

    # -- a4..a6 (:383-544) ---------------------------------------------------------
    def probability_of_match(self, state, blob, feature):
        r = self._probe(_state_pose(state), feature.mean, feature.covar, _blob_row(blob))
        return float(r["probability_of_match"])

    def prob_position_match(self, f_mean, f_covar, s_x, s_y, bearing):
        cov = np.identity(5)
        cov[:2, :2] = np.asarray(f_covar, dtype=np.float64)[0:2, 0:2]
        mean = np.zeros(5)
        mean[:2] = np.asarray(f_mean, dtype=np.float64)[:2]
        r = self._probe((float(s_x), float(s_y), 0.0), mean, cov, (float(bearing), 0.0, 0.0, 0.0))
        return float(r["prob_position_match"])

    def closest_point(self, f_x, f_y, s_x, s_y, obs_bearing):
        r = self._probe((float(s_x), float(s_y), 0.0), (float(f_x), float(f_y), 0, 0, 0), np.identity(5),
                        (float(obs_bearing), 0.0, 0.0, 0.0))
        return (float(r["closest_point"][0]), float(r["closest_point"][1]))

    def prob_color_match(self, f_mean, f_covar, blob):
        cov = np.identity(5)
        cov[2:, 2:] = np.asarray(f_covar, dtype=np.float64)[2:, 2:]
        z = _blob_row(blob)
        r = self._probe((0.0, 0.0, 0.0), np.asarray(f_mean, dtype=np.float64), cov, z)
        return float(r["prob_color_match"])

    # -- a7..a11 (:748-877) ----------------------------------------------------------
    def _probe_feature(self, feature_id, blob=None, Qt=None):
        f = self.get_feature_by_id(feature_id)
        z = _blob_row(blob) if blob is not None else np.array([0.0, f.mean[2], f.mean[3], f.mean[4]], dtype=np.float64)
        return self._probe(_state_pose(self.state), f.mean, f.covar, z, Qt)

    def generate_measurement(self, featureid):
        r = self._probe_feature(featureid)
        f = self.get_feature_by_id(featureid)
        bobby = Blob()
        bobby.bearing = float(r["zhat"][0])
        bobby.color.r = f.mean[2]
        bobby.color.g = f.mean[3]
        bobby.color.b = f.mean[4]
        return bobby

    def measurement_jacobian(self, feature_id):
        r = self._probe_feature(feature_id)
        H = np.zeros((4, 5))
        H[0, 0], H[0, 1] = r["H0"]
        H[1, 2] = H[2, 3] = H[3, 4] = 1.0
        return H

    def measurement_covariance(self, bigH, feature_id, Qt):
        """Q = H Sigma H' + Qt (:804-819).  H is re-derived on the device from the particle
        state, which is what ``measurement_jacobian`` returned."""
        return self._probe_feature(feature_id, Qt=Qt)["Q"]

    def kalman_gain(self, feature_id, bigH, Qinv):
        """K = Sigma H' Q^-1 (:821-833); Qt is recovered from the caller's Q^-1."""
        Q0 = self._probe_feature(feature_id, Qt=np.zeros((4, 4)))["Q"]
        Qt = np.linalg.inv(np.asarray(Qinv, dtype=np.float64)) - Q0
        return self._probe_feature(feature_id, Qt=Qt)["K"]

    def importance_factor(self, bigQ, blob, pseudoblob):
        """(2 pi ||Q||_F)^-1/2 exp(-1/2 d' Q^-1 d) (:835-849) for caller-supplied matrices.
        Inside the filter this factor is computed by k_observe; this scalar helper exists
        for scripts that call it directly and is a few NumPy flops, as in the reference."""
        v1 = pow(2.0 * math.pi * np.linalg.norm(bigQ), -0.5)
        delz = _blob_row(blob) - _blob_row(pseudoblob)
        return v1 * math.exp(-0.5 * np.dot(np.dot(delz.T, np.linalg.inv(bigQ)), delz))

    def no_match_weight(self):
        return NO_MATCH_WEIGHT

    # -- f4: new-landmark machinery (:546-746) ------------------------------------------------
    # Host bookkeeping per unmatched blob, as in the reference (not part of the data-parallel path: inside the
    # filter the device only applies the 0.1 weight of :95).  Restated with the reference's arithmetic order so
    # that its own unit tests (test_prkt_ros2.py:228-381) hold exactly -- including the behaviour that makes the
    # machinery a dead end there: find_nearest_reading walks ``potential_features`` (never filled by the filter)
    # and returns the nearest entry's key, which is negative or 0, so add_hypothesis always files an orphan.
    def add_hypothesis(self, state, blob):
        """:546-564."""
        pair_id = self.find_nearest_reading(state, blob)
        if pair_id > 0:
            self.add_new_feature(pair_id, state, blob)
        else:
            self.add_orphaned_reading(state, blob)

    def find_nearest_reading(self, state, blob):
        """:566-590: key of the stored reading at the smallest reading distance (first one on ties), 0 if none
        is at a finite distance."""
        best_id, best = 0, float('inf')
        for id_, reading in self.potential_features.items():
            d = self.reading_distance_function(reading[0], reading[1], state, blob)
            if d < best:
                best, best_id = d, id_
        return best_id

    def reading_distance_function(self, state1, blob1, state2, blob2):
        """:592-609: colour distance of two readings whose rays cross, else inf."""
        x1, y1, h1 = _state_pose(state1)
        x2, y2, h2 = _state_pose(state2)
        if not self.ray_intersect(x1, y1, blob1.bearing + h1, x2, y2, blob2.bearing + h2):
            return float('inf')
        return self.color_distance(blob1, blob2)

    def ray_intersect(self, x1, y1, b1, x3, y3, b3):
        """:611-643: do the half-lines (x1, y1, b1) and (x3, y3, b3) meet (both ray parameters >= 0)."""
        ax, ay = math.cos(b1), math.sin(b1)
        bx, by = math.cos(b3), math.sin(b3)
        cross = ay * bx - ax * by
        if cross == 0:
            return False
        v = (ax * y3 - ay * x3 + ay * x1 - ax * y1) / cross
        if abs(ay) < abs(ax):
            u = (x3 + bx * v - x1) / ax
        else:
            u = (y3 + by * v - y1) / ay
        return u >= 0 and v >= 0

    @staticmethod
    def _ray_determinant(b1, b3):
        """The determinant ray_intersect forms for two world bearings: minus the sine of the angle between the rays."""
        return math.sin(b1) * math.cos(b3) - math.cos(b1) * math.sin(b3)

    @staticmethod
    def _triangulated_covariance(x1, y1, t1, x3, y3, t3, ox, oy, q00):
        """(Pxx, Pxy, Pyy) of the crossing (ox, oy) of the lines (x1, y1, t1) and (x3, y3, t3) whose bearings carry the variance
        q00: J diag(q00, q00) J' with dX/dt1 = (u / sd) d3, dX/dt3 = -(v / sd) d1 (landmark_init="triangulated"; pk_grow_init)."""
        s1, c1, s3, c3 = math.sin(t1), math.cos(t1), math.sin(t3), math.cos(t3)
        sd = s3 * c1 - c3 * s1
        u = (ox - x1) * c1 + (oy - y1) * s1
        v = (ox - x3) * c3 + (oy - y3) * s3
        a, b = u / sd, v / sd
        aa, bb = a * a, b * b
        return (q00 * (aa * (c3 * c3) + bb * (c1 * c1)), q00 * (aa * (c3 * s3) + bb * (c1 * s1)),
                q00 * (aa * (s3 * s3) + bb * (s1 * s1)))

    def color_distance(self, blob1, blob2):
        """:645-654: Euclidean distance of the two colours."""
        return math.sqrt(math.pow(blob1.color.r - blob2.color.r, 2) + math.pow(blob1.color.g - blob2.color.g, 2) +
                         math.pow(blob1.color.b - blob2.color.b, 2))

    def add_new_feature(self, old_id, state, blob):
        """:656-686: a potential feature (negative id) where the stored reading old_id and this one cross, mean
        colour of the two, identity covariance."""
        old_state, old_blob = self.hypothesis_set[old_id]
        x, y = self.cross_readings((old_state, old_blob), (state, blob))
        mean = np.array([x, y, (old_blob.color.r + blob.color.r) / 2, (old_blob.color.g + blob.color.g) / 2,
                         (old_blob.color.b + blob.color.b) / 2])
        self.potential_features[-self.next_id] = Feature(mean=mean, covar=np.identity(5))
        self.next_id += 1

    def cross_readings(self, old_reading, new_reading):
        """:688-737: intersection of the two LINES through the readings (also behind the observers), None when
        they are parallel.  Line-line intersection through two points each, one unit step along the ray apart."""
        x1, y1, h1 = _state_pose(old_reading[0])
        x3, y3, h3 = _state_pose(new_reading[0])
        return self._cross_lines(x1, y1, h1 + old_reading[1].bearing, x3, y3, h3 + new_reading[1].bearing)

    @staticmethod
    def _cross_lines(x1, y1, h1, x3, y3, h3):
        """The arithmetic of cross_readings on plain numbers (world-frame bearings h1, h3)."""
        x2, y2 = x1 + math.cos(h1), y1 + math.sin(h1)
        x4, y4 = x3 + math.cos(h3), y3 + math.sin(h3)
        d12, d34 = x1 * y2 - y1 * x2, x3 * y4 - x4 * y3
        den = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
        if den == 0:
            return None
        return ((d12 * (x3 - x4) - (x1 - x2) * d34) / den, (d12 * (y3 - y4) - (y1 - y2) * d34) / den)

    def add_orphaned_reading(self, state, blob):
        """:739-746."""
        self.hypothesis_set[self.next_id] = ((state, blob,))
        self.next_id += 1



def _check_landmark_init(landmark_init, min_parallax, new_landmarks, who="FastSLAM"):
    """(name, min_parallax) of the landmark_init / min_parallax keywords, or ValueError -- before any device work."""
    if landmark_init not in _lib.LANDMARK_INITS:
        raise ValueError("%s(landmark_init=%r): 'reference' (default) or 'triangulated'" % (who, landmark_init))
    try:
        angle = float(min_parallax)
    except (TypeError, ValueError):
        raise ValueError("%s(min_parallax=%r): an angle in [0, pi / 2] radians" % (who, min_parallax))
    if not (0.0 <= angle <= math.pi / 2):  # (a NaN fails)
        raise ValueError("%s(min_parallax=%r): an angle in [0, pi / 2] radians" % (who, min_parallax))
    if landmark_init != "reference" and not new_landmarks:
        raise ValueError("%s(landmark_init=%r): new landmarks are initialised by a growing map (new_landmarks=True)" % (who, landmark_init))
    return landmark_init, angle


# ----------------------------------------------------------------------------- new-landmark bookkeeping: arrays <-> lists
def _nl_unpack(cnt, rd, sid, L0):
    """pk_grow_download's arrays of n particles as the host lists of the growing mode."""
    n = cnt.shape[0]
    return dict(
        hyp=[[(int(r[0]),) + tuple(float(v) for v in r[1:]) for r in rd[i, :cnt[i, 0]]] for i in range(n)],
        next_id=[int(v) for v in cnt[:, 2]], used=[int(v) for v in cnt[:, 1]],
        slot_id=[{L0 + k: int(sid[i, k]) for k in range(cnt[i, 1])} for i in range(n)],
        dropped=int(cnt[:, 3].sum()))


def _nl_pack(hyp, next_id, used, slot_id, L0, S, R):
    """... and back: (counters (n, 4), readings (n, R, 8), slot ids (n, S)) for pk_grow_upload."""
    n = len(hyp)
    cnt = np.zeros((n, 4), dtype=np.int32)
    rd = np.zeros((n, R, 8))
    sid = np.zeros((n, S), dtype=np.int32)
    for i in range(n):
        cnt[i, :3] = (len(hyp[i]), used[i], next_id[i])
        if hyp[i]:
            rd[i, :len(hyp[i])] = np.asarray(hyp[i], dtype=np.float64)
        for slot, fid in slot_id[i].items():
            sid[i, slot - L0] = fid
    return cnt, rd, sid


def _nl_snapshot(nl):
    """The bookkeeping as plain numeric arrays (a snapshot never needs pickle to load): every particle's orphaned readings
    (8 numbers each) back to back with per-particle offsets, the id counters, and the (particle, slot, id) triples of the
    spare slots in use."""
    offs = np.zeros(len(nl["hyp"]) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(h) for h in nl["hyp"]])
    flat = [rd for h in nl["hyp"] for rd in h]
    return dict(
        nl_readings=np.asarray(flat, dtype=np.float64).reshape(len(flat), 8),
        nl_offsets=offs,
        nl_next_id=np.asarray(nl["next_id"], dtype=np.int64),
        nl_used=np.asarray(nl["used"], dtype=np.int64),
        nl_slot_id=np.asarray([(i, s, v) for i, d in enumerate(nl["slot_id"]) for s, v in sorted(d.items())],
                              dtype=np.int64).reshape(-1, 3))


def _nl_snapshot_arrays(cnt, rd, sid, L0):
    """_nl_snapshot straight from pk_grow_download's arrays (no per-particle Python objects: a snapshot of 10^5 particles)."""
    n, used = cnt[:, 0].astype(np.int64), cnt[:, 1].astype(np.int64)
    offs = np.zeros(cnt.shape[0] + 1, dtype=np.int64)
    offs[1:] = np.cumsum(n)
    keep = np.arange(rd.shape[1])[None, :] < n[:, None]
    in_use = np.arange(sid.shape[1])[None, :] < used[:, None]
    ii, kk = np.nonzero(in_use)
    return dict(nl_readings=np.ascontiguousarray(rd[keep], dtype=np.float64).reshape(-1, 8), nl_offsets=offs,
                nl_next_id=cnt[:, 2].astype(np.int64), nl_used=used,
                nl_slot_id=np.stack([ii, L0 + kk, sid[in_use].astype(np.int64)], axis=1).astype(np.int64).reshape(-1, 3))


def _nl_arrays_from_snapshot(d, P, L0, S, R):
    """... and back: (counters, readings, slot ids) for pk_grow_upload from a CHECKED snapshot."""
    offs = np.asarray(d["nl_offsets"], dtype=np.int64)
    n = np.diff(offs)
    cnt = np.zeros((P, 4), dtype=np.int32)
    cnt[:, 0], cnt[:, 1], cnt[:, 2] = n, d["nl_used"], d["nl_next_id"]
    rd = np.zeros((P, R, 8))
    rd[np.arange(R)[None, :] < n[:, None]] = np.asarray(d["nl_readings"], dtype=np.float64).reshape(-1, 8)
    sid = np.zeros((P, S), dtype=np.int32)
    t = np.asarray(d["nl_slot_id"], dtype=np.int64).reshape(-1, 3)
    sid[t[:, 0], t[:, 1] - L0] = t[:, 2]
    return cnt, rd, sid


def _nl_check_snapshot(d, P, L0, L, spare, ring=None):
    """Raises ValueError unless d's nl_* arrays fit a filter of P particles, landmarks [L0, L) spare, rings of `ring` readings."""
    offs, rd = d["nl_offsets"], d["nl_readings"]
    used, slot_id = d["nl_used"], d["nl_slot_id"]
    if (offs.shape != (P + 1,) or offs[0] != 0 or np.any(np.diff(offs) < 0) or rd.shape != (int(offs[-1]), 8)
            or d["nl_next_id"].shape != (P,) or used.shape != (P,) or slot_id.ndim != 2 or slot_id.shape[1] != 3):
        raise ValueError("snapshot: malformed new-landmark bookkeeping")
    if (np.any(used < 0) or np.any(used > spare) or np.any(slot_id[:, 0] < 0) or np.any(slot_id[:, 0] >= P)
            or np.any(slot_id[:, 1] < L0) or np.any(slot_id[:, 1] >= L)):
        raise ValueError("snapshot: new-landmark bookkeeping names particles / spare slots this filter does not have")
    if ring is not None and P and int(np.diff(offs).max()) > ring:
        raise ValueError("snapshot: a particle holds %d orphaned readings, this filter keeps %d (reading_capacity)"
                         % (int(np.diff(offs).max()), ring))


def _nl_restore(d, P):
    """(hyp, next_id, used, slot_id) lists from a checked snapshot."""
    offs, rd = d["nl_offsets"], d["nl_readings"]

    def reading(r):  # (id, x, y, heading, bearing, r, g, b): the id is an integer
        return (int(r[0]),) + tuple(float(v) for v in r[1:])

    slot_ids = [dict() for _ in range(P)]
    for i, slot, fid in d["nl_slot_id"]:
        slot_ids[int(i)][int(slot)] = int(fid)
    return ([[reading(r) for r in rd[offs[i]:offs[i + 1]]] for i in range(P)], [int(v) for v in d["nl_next_id"]],
            [int(v) for v in d["nl_used"]], slot_ids)


# =============================================================================
class _ParticleList(list):
    """``FastSLAM.particles``: list-like view of the particles held in HBM."""

    def __init__(self, owner):
        super().__init__()
        self._o = owner

    def __len__(self):
        return self._o.num_particles

    def __iter__(self):
        for i in range(len(self)):
            yield self._o._particle_view(i)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._o._particle_view(j) for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("particle index out of range")
        return self._o._particle_view(i)

    def __setitem__(self, i, particle):
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("particle index out of range")
        self._o._store_particle(i, particle)

    def __repr__(self):
        return "<%d particles on GPU %d>" % (len(self), self._o._device)


class FastSLAM(object):
    """prkt_core_v2.py:37-276 on an MI355X.

    FastSLAM(preset_features=[], num_particles=50, device=0, weight_domain="linear",
             rng="global", seed=0, publish_debug=None)

    rng="global": motion noise from ``numpy.random`` and the resample draw from
    ``random.random()`` -- the reference's own streams, so ``np.random.seed(s);
    random.seed(s)`` reproduces the reference bit for bit in the draws;
    rng="device": Philox noise generated on the GPU (no host->device upload).

    new_landmarks=True (with spare_landmarks=S slots per particle): the new-landmark initialisation of :546-746 and the
    potential-feature rule of :109-118, made to work (in the reference ``find_nearest_reading`` walks
    ``potential_features`` where the readings are in ``hypothesis_set``, so nothing is ever paired): an unmatched blob is
    paired with the nearest stored reading of the particle -- rays crossing, colour distance below ``pair_threshold`` --
    and becomes a potential feature at the crossing, else it is stored as an orphaned reading.  Matching, the EKF
    update, the 0.1 weight of a potential feature and its promotion past update_count 5 run in the device kernels (a
    flag in the landmark's count word).  The per-unmatched-blob bookkeeping runs on the device too (bookkeeping="device",
    the default: one kernel behind every observe, pk_grow_enable; each particle keeps up to ``reading_capacity`` orphaned
    readings in HBM, ``readings_dropped()`` counts what did not fit) -- nothing per particle crosses to the host in a step;
    bookkeeping="host" is the per-particle host loop of the reference (and the only one on the dense layout).
    ``reading_max_age=A`` / ``potential_max_idle=M`` (device bookkeeping, one GPU; 0: never, the default): behind every scan's
    bookkeeping each particle drops the readings at the head of its ring that are A scans old or older and retires the potential
    features that went unmatched for M scans, whose spare slots are free again (pk_grow_retire); ``retired()`` counts both.
    ``view=(half_fov, r_min, r_max)`` with ``confirmed_max_misses=C`` (needs one of the two thresholds above; default: none): the
    sensor's field for that pass (pk_grow_view; DESIGN.md section 9, "A field of view for retirement").  An unmatched feature ages
    only in the scans in which its position mean lies within half_fov radians of the particle's heading and between r_min and
    r_max of its position (r_max may be inf) -- a feature the camera points away from is left alone -- and a promoted feature is
    retired after C such misses in a row (0: never).  ``view_stats()`` reads the pass's counters.  The view is configuration, like
    the thresholds: no snapshot holds it.
    ``landmark_init="triangulated"`` (default "reference": the rule above) with ``min_parallax`` (radians in [0, pi / 2], default
    0.2): a stored reading is paired only if its ray meets the blob's at min_parallax or more -- a blob with no such reading is
    stored, so that a later scan pairs with it across a wider baseline -- and the new feature starts with the triangulation's own
    position covariance, J diag(Qt[0][0], Qt[0][0]) J' over the two bearings, in place of the identity (pk_grow_init; DESIGN.md
    section 9, "Parallax-gated pairing").  Both bookkeeping modes apply it, ``save_state`` writes both values and ``load_state``
    takes them from the snapshot (one without them: "reference").
    ``record_ids`` (default: only with bookkeeping="host"): keep ``last_ids`` / ``last_ancestors`` of every step.

    record_path=T (default 0: off): every resample records the generation it worked on and its ancestors in a ring of the last
    T steps on the device (pk_path_enable: 28 bytes per particle and step); ``path_summary()`` is the smoothed path over the
    surviving lineages with the number of distinct ancestors left per step, ``particle_paths(indices)`` the paths of single
    particles, ``path_summary(weighting="weights")`` the path by the particles' weights (between the resamples of an adaptively
    resampled filter) and ``best_path()`` that of the most likely particle.  One GPU only: with devices=[several] it is refused.
    settle_path=E (default None: off; True: max(1, T // 4)): the ring never overwrites -- the record that fills it settles its
    oldest E rows into a trunk of 104 bytes per step on the device (pk_path_trunk_enable), and ``full_path()`` is the path of the
    whole run, trunk, ring and current generation, in bounded memory.  Needs record_path, E <= T.

    resample_threshold=theta (default None: resample behind every scan, as the reference does): adaptive resampling -- the
    filter resamples only when the effective sample size of its weights falls below theta * num_particles, decided on the device
    (pk_resample_adaptive); otherwise the particles stay and their weights carry over into the next scan.  ``summary()`` is
    then the WEIGHTED pose, ``pose_summary()`` its full form, ``map_summary()`` weights by default, ``resample_stats()`` says
    what the last step decided, and ``last_ancestors`` is the identity on a kept step.  The resample draw is taken at every
    step, kept or not, so the random stream does not depend on the decisions.  One GPU only, as record_path.

    motion="odometry" (default "twist": the reference's commanded twist with its hard-wired noise): the particles move by
    ``odom_motion_update(odom)`` alone -- the reference's empty stub (:140-146), finished.  Every message after the first moves
    ALL particles by the change between the previous message's pose and its own: the odometry motion model of Probabilistic
    Robotics, Table 5.6 (rotate, translate, rotate; pk_odom_delta, pk_motion_odom), whose noise grows with the motion through
    ``odom_alphas=(a1, a2, a3, a4)``: sigma_rot^2 = a1 rot^2 + a2 trans^2, sigma_trans^2 = a3 trans^2 + a4 (rot1^2 + rot2^2).
    A translation below ``odom_min_trans`` (0.01 m) is a turn in place: it is applied along the current heading, which puts the
    position off by 2 trans sin(phi / 2), phi the angle between the heading and the dropped direction -- at most odom_min_trans
    within 60 degrees of the heading, below 2 odom_min_trans always; the heading stays exact.  ``motion_update(twist)`` then only records the control, and ``cam_cb`` applies the scan to
    the poses as the last odometry message left them.  A robot that stood still launches nothing and consumes no draw.
    ``motion_model(particle, twist, dt)`` stays the twist model.  Works with devices=[several] too.

    proposal="measurement" (default "motion": every pose is drawn from the motion model alone and the scan only weighs it,
    FastSLAM 1.0; that code path is untouched): with measurement_model="bearing", ``cam_cb`` draws every pose from the motion model
    CONDITIONED on its scan (FastSLAM 2.0; pk_propose, pk_propose_odom; DESIGN.md section 4, "The measurement-informed proposal") --
    one call in place of the move and the observe, with the same dt bookkeeping and draw counter.  In odometry mode
    ``odom_motion_update`` only stores the message, and ``cam_cb`` moves by the change since the pose it last moved up to.  One GPU,
    preset maps only (no new_landmarks) unless proposal_grow=True.  ``record_ids=True`` keeps every step's settled ids in
    ``last_ids`` (one download per step).

    measurement_model="bearing" (default "reference": the reference's model, quirks included): the textbook robot-frame bearing
    model -- wrapped bearing differences in the gate and the innovation, the blob's ray turned by the heading, H = (-dy / q, dx / q),
    the Gaussian density with det Q as the weight (pk_set_measurement_model; DESIGN.md section 4, "The bearing model").  It is the
    model that localises a robot that turns.  Its scans take the general kernels; one GPU only, the compact layout only.
    ``save_state`` writes the model's name and ``load_state`` refuses a snapshot taken with the other one.

    range_noise=(sigma0, sigma1) (default None; measurement_model="bearing", proposal="motion", a preset map): scans may carry a
    range per blob -- a depth camera, a stereo pair, a lidar front end -- for all blobs or for some (pk_scan_ranges; DESIGN.md section
    4, "Range-bearing scans").  A scan is message objects with an optional ``range`` attribute (absent, None or NaN: this blob has
    none), or a (B, 5) array (bearing, r, g, b, range).  A range rho gets the variance (sigma0 + sigma1 rho)^2, formed on the host.
    A ranged blob is associated at its measured point and updates its landmark with the 2-D measurement (bearing, range): landmarks
    of one colour on one ray are told apart, and a landmark's depth no longer waits for parallax.  The pose estimate does not gain
    by it on the drives measured.  With range_noise=None a (B, 5) array is a ValueError, and a ``range`` attribute of message objects
    is IGNORED.  Ranges are not state: snapshots do not change.

    proposal_ranges=True (default False; with proposal="measurement" and range_noise=(sigma0, sigma1)): the ranges enter the
    measurement-informed proposal (pk_proposal_ranges; DESIGN.md section 4, "Ranges in the proposal") -- a ranged blob is associated
    at its measured point at the predicted pose and conditions the pose draw, the weight and the update as the 2-D measurement
    (bearing, range); a blob without a range is the bearing-only proposal's, blob by blob.  Without it range_noise and
    proposal="measurement" stay a ValueError; with it and no range_noise, or with proposal="motion", it is one too.

    grow_ranges=True (default False; with range_noise=(sigma0, sigma1), new_landmarks=True, spare_landmarks > 0, the device
    bookkeeping and proposal="motion"): a growing map takes ranged scans (pk_grow_ranges; DESIGN.md section 9, "Single-sighting
    initialisation").  Matched blobs are associated and updated as on a preset map; an unmatched blob with a range becomes a potential
    feature at once, at its measured point with the covariance q_rho u u' + rho^2 Qt[0][0] n n', and stores no reading; one without a
    range goes through ``landmark_init``'s rule.  Without it range_noise and new_landmarks=True stay a ValueError; with it, a missing
    range_noise, a preset map, bookkeeping="host" or proposal="measurement" is one.  ``save_state`` writes the flag when it is set
    and ``load_state`` takes it from the snapshot (one without it: off).  One GPU (the bearing model's).

    proposal_grow=True (default False; with proposal="measurement", new_landmarks=True, spare_landmarks > 0 and the device
    bookkeeping): the measurement-informed proposal on a growing map (pk_proposal_grow; DESIGN.md section 4, "The proposal on growing
    maps").  Every pose is drawn conditioned on the scan's matches to CONFIRMED landmarks; a match to a potential feature is updated
    and weighs log 0.1; the unmatched blobs then go through ``landmark_init``'s rule at the SAMPLED pose, and the retirement pass
    follows.  range_noise then needs proposal_ranges=True and grow_ranges=True together: a ranged unmatched blob becomes a potential
    feature at once.  Without the keyword proposal="measurement" with new_landmarks=True stays a ValueError; with it,
    proposal="motion", a preset map, no spare slot, bookkeeping="host" or several devices is one.  In odometry mode a scan with no
    new odometry is the plain growing observe.  Snapshots do not carry the flag (they do not carry ``proposal`` either).  One GPU.

    association="unique" (default "ml"): unique data association (pk_assoc_unique; DESIGN.md section 4, "Unique association" -- the
    reference's unwritten "Version 2", prkt_core_v2.py:317-351).  Every scan's maximum-likelihood ids are settled per particle so that
    no landmark keeps more than one blob: the pairs are taken greedily by match probability, then scan order, then landmark index,
    and a blob that loses everywhere is unmatched -- on a growing map it becomes a reading or a feature.  ``last_ids`` /
    ``record_ids`` carry the settled ids; ``association_stats()`` returns the last scan's counters.  Both measurement models,
    range_noise and growing maps take it; proposal="measurement", several devices or an unknown name is a ValueError.
    Configuration, not state: snapshots do not carry it.
    """

    EMPTY_COLOUR = 2.0 ** 100  # colour of a spare slot that holds nothing yet: fails every colour gate (:441), exact in float32

    def __new__(cls, *args, **kwargs):
        # FastSLAM(preset_features, devices=[0, 1, ...]): the same class surface with the particles sharded over several
        # GPUs, one child process per device (multi.py; SURVEY section 5's `devices=` keyword).  The arguments are bound
        # against FastSLAM's OWN signature -- positional ones included -- and forwarded with FastSLAM's defaults (weight_domain
        # "linear", rng "global"); what the sharded facade cannot do is refused, not dropped.
        extra = {k: kwargs.pop(k) for k in ("backend", "_shard_factory") if k in kwargs}
        try:
            ba = _inspect.signature(cls.__init__).bind(None, *args, **kwargs)
        except TypeError:
            return super(FastSLAM, cls).__new__(cls)  # __init__ raises the same TypeError with its own wording
        ba.apply_defaults()
        a = ba.arguments
        _check_landmark_init(a["landmark_init"], a["min_parallax"], a["new_landmarks"])
        _check_association(a["association"], a["proposal"], a.get("devices"))
        _check_proposal_grow(bool(a["proposal_grow"]), a["proposal"], a["new_landmarks"], a["spare_landmarks"], a["bookkeeping"],
                             a.get("devices"), a["range_noise"], bool(a["proposal_ranges"]), bool(a["grow_ranges"]))
        _check_range_noise(a["range_noise"], a["measurement_model"], a["proposal"], a["new_landmarks"],
                           proposal_ranges=bool(a["proposal_ranges"]), grow_ranges=bool(a["grow_ranges"]),
                           proposal_grow=bool(a["proposal_grow"]))
        _check_grow_ranges(a["grow_ranges"], a["spare_landmarks"], a["bookkeeping"])
        _check_view(a["view"], a["confirmed_max_misses"], a["reading_max_age"], a["potential_max_idle"], a["new_landmarks"],
                    a["spare_landmarks"], a["bookkeeping"], a.get("devices"))
        devices = a.get("devices")
        if devices is not None and len(list(devices)) > 1:
            from .multi import ShardedFastSLAM

            if a["new_landmarks"] and a["bookkeeping"] != "device":
                raise ValueError("FastSLAM(devices=[...]): the new-landmark bookkeeping of several GPUs lives on the devices "
                                 "(bookkeeping='device'): host lists cannot follow a particle from one GPU to another")
            if a["device"] not in (0, list(devices)[0]):
                raise ValueError("FastSLAM: give either device= or devices=, not both")
            if a["proposal"] != "motion":
                raise ValueError("FastSLAM(devices=[...], proposal=%r): the measurement-informed proposal runs on one GPU; an "
                                 "unknown name is refused the same way" % (a["proposal"],))
            if a["measurement_model"] != "reference":
                raise ValueError("FastSLAM(devices=[...], measurement_model=%r): the bearing model runs on one GPU -- the ranged "
                                 "and split observes of the sharded step have no kernel for it; an unknown name is refused the "
                                 "same way" % (a["measurement_model"],))
            if a["settle_path"]:
                raise ValueError("FastSLAM(devices=[...], settle_path=...): the path is recorded and settled on one GPU only -- "
                                 "lineages across ranks are out of scope")
            if a["record_path"]:
                raise ValueError("FastSLAM(devices=[...], record_path=...): the path is recorded on one GPU only -- lineages "
                                 "across ranks are out of scope (the sharded resample is refused on a recording filter)")
            if a["resample_threshold"] is not None:
                raise ValueError("FastSLAM(devices=[...], resample_threshold=...): adaptive resampling is for one GPU -- the "
                                 "verdict of a sharded filter needs its weight sums all-reduced, which is out of scope")
            if a["reading_max_age"] or a["potential_max_idle"]:
                raise ValueError("FastSLAM(devices=[...], reading_max_age=... / potential_max_idle=...): readings and features are "
                                 "retired on one GPU only -- a particle's record carries no clocks from one rank to another")
            return ShardedFastSLAM(a["preset_features"], num_particles=a["num_particles"], devices=list(devices),
                                   weight_domain=a["weight_domain"], rng=a["rng"], seed=a["seed"],
                                   publish_debug=a["publish_debug"], new_landmarks=a["new_landmarks"],
                                   spare_landmarks=a["spare_landmarks"], pair_threshold=a["pair_threshold"],
                                   reading_capacity=a["reading_capacity"], motion=a["motion"], odom_alphas=a["odom_alphas"],
                                   odom_min_trans=a["odom_min_trans"], landmark_init=a["landmark_init"],
                                   min_parallax=a["min_parallax"], **extra)
        if extra:
            raise TypeError("FastSLAM: %s only apply with devices=[...] naming several GPUs" % ", ".join(sorted(extra)))
        return super(FastSLAM, cls).__new__(cls)

    def __init__(self, preset_features=[], num_particles=50, device=0, weight_domain="linear", rng="global",
                 seed=0, publish_debug=None, new_landmarks=False, spare_landmarks=0, pair_threshold=30.0, devices=None,
                 bookkeeping="device", reading_capacity=64, record_ids=None, record_path=0, resample_threshold=None,
                 reading_max_age=0, potential_max_idle=0, settle_path=None, motion="twist", odom_alphas=_odom.DEFAULT_ALPHAS,
                 odom_min_trans=_odom.DEFAULT_MIN_TRANS, measurement_model="reference", proposal="motion",
                 landmark_init="reference", min_parallax=0.2, range_noise=None, proposal_ranges=False, grow_ranges=False,
                 proposal_grow=False, association="ml", view=None, confirmed_max_misses=0):
        self._landmark_init, self._min_parallax = _check_landmark_init(landmark_init, min_parallax, new_landmarks)
        self._association = _check_association(association, proposal, devices)
        if measurement_model not in _lib.MEASUREMENT_MODELS:
            raise ValueError("FastSLAM(measurement_model=%r): 'reference' (default) or 'bearing'" % (measurement_model,))
        self._proposal_grow = _check_proposal_grow(bool(proposal_grow), proposal, new_landmarks, spare_landmarks, bookkeeping, devices,
                                                   range_noise, bool(proposal_ranges), bool(grow_ranges))
        self._range_noise = _check_range_noise(range_noise, measurement_model, proposal, new_landmarks,
                                               proposal_ranges=bool(proposal_ranges), grow_ranges=bool(grow_ranges),
                                               proposal_grow=self._proposal_grow)
        self._proposal_ranges = bool(proposal_ranges)
        self._grow_ranges = _check_grow_ranges(grow_ranges, spare_landmarks, bookkeeping)
        if proposal not in ("motion", "measurement"):
            raise ValueError("FastSLAM(proposal=%r): 'motion' (default) or 'measurement'" % (proposal,))
        if proposal == "measurement" and measurement_model != "bearing":
            raise ValueError("FastSLAM(proposal='measurement'): the measurement-informed proposal needs measurement_model='bearing' "
                             "-- the reference model's Jacobian is not one")
        if proposal == "measurement" and new_landmarks and not self._proposal_grow:
            raise ValueError("FastSLAM(proposal='measurement', new_landmarks=True): growing maps are found by the plain step "
                             "(proposal='motion')")
        self._model = measurement_model
        self._proposal = proposal
        self._proposal_ids = proposal == "measurement" and bool(record_ids)  # record_ids=True: cam_cb keeps every step's settled ids
        self._odom_applied = None  # proposal='measurement', odometry mode: the odometry pose the particles were last moved up to
        self._motion, self._odom_alphas, self._odom_min_trans = _odom.check_keywords(motion, odom_alphas, odom_min_trans)
        self._odom_prev = None  # the last odometry pose (x, y, heading); None: the next message is the first
        if devices is not None and len(list(devices)) == 1:
            device = list(devices)[0]
        self._retire = (int(reading_max_age), int(potential_max_idle))
        if min(self._retire) < 0:
            raise ValueError("reading_max_age and potential_max_idle must be numbers of scans >= 0")
        if any(self._retire) and not (new_landmarks and int(spare_landmarks) > 0 and bookkeeping == "device"):
            raise ValueError("FastSLAM(reading_max_age=... / potential_max_idle=...): readings and features are retired by the device "
                             "bookkeeping of a growing map (new_landmarks=True, spare_landmarks > 0, bookkeeping='device'), not by "
                             "bookkeeping='host'")
        self._view, self._confirmed_max_misses = _check_view(view, confirmed_max_misses, reading_max_age, potential_max_idle,
                                                              new_landmarks, spare_landmarks, bookkeeping, devices)
        self._threshold = None if resample_threshold is None else adaptive.threshold_value(resample_threshold)
        self._lock = threading.RLock()
        self.last_control = Twist()
        self.last_update = msgs.now()
        self.num_particles = int(num_particles)
        self._device = int(device)
        self._features = list(preset_features)
        self._ids = list(range(1, len(self._features) + 1))  # load_feature_list :294-299
        L = len(self._features)
        self._grow = bool(new_landmarks)
        self._spare = int(spare_landmarks) if self._grow else 0
        self._pair_threshold = float(pair_threshold)
        self._L0 = L
        self._filter = _lib.DeviceFilter(self.num_particles, L + self._spare, device=self._device)
        if self._model != "reference":
            self._filter.set_measurement_model(self._model)
        if self._proposal_ranges:
            self._filter.proposal_ranges(True)
        if self._proposal_grow:
            self._filter.proposal_grow(True)
        if self._association == "unique":
            self._filter.assoc_unique(True)
        if L + self._spare:
            means = np.zeros((L + self._spare, 5))
            covs = np.tile(np.identity(5).reshape(25), (L + self._spare, 1))
            imm = np.zeros(L + self._spare, dtype=np.uint8)
            if L:
                means[:L] = np.array([np.asarray(f.mean, dtype=np.float64).reshape(5) for f in self._features])
                covs[:L] = np.array([np.asarray(f.covar, dtype=np.float64).reshape(25) for f in self._features])
                imm[:L] = np.array([bool(f.__immutable__) for f in self._features], dtype=np.uint8)
            means[L:, 2:] = self.EMPTY_COLOUR
            self._filter.upload_map(means, covs, imm)
        P = self.num_particles
        if bookkeeping not in ("device", "host"):
            raise ValueError("bookkeeping must be 'device' or 'host'")
        # the per-particle bookkeeping of the growing mode (follows the particles through every resample): on the device
        # (pk_grow_enable; the four views below download it when asked) or in host lists
        self._nl_device = self._grow and self._spare > 0 and bookkeeping == "device"
        self._nl_cache = None
        if self._nl_device:
            try:
                self._filter.grow_enable(L, int(reading_capacity), self._pair_threshold)
            except _lib.PkError as e:
                if e.status != _lib.PK_ERR_STATE:
                    raise
                self._filter.close()
                raise ValueError("%s -- FastSLAM(..., bookkeeping='host') keeps the new-landmark bookkeeping on the host, on any layout" % e)
            if any(self._retire):
                self._filter.grow_retire(*self._retire)
            if self._view is not None:
                self._filter.grow_view(self._view[0], self._view[1], self._view[2], self._confirmed_max_misses)
            if self._landmark_init != "reference":
                self._filter.grow_init(self._landmark_init, self._min_parallax)
            if self._grow_ranges:
                self._filter.grow_ranges(True)
        else:
            self._nl_host = dict(
                hyp=[[] for _ in range(P)],          # orphaned readings: (id, x, y, heading, bearing, r, g, b)  (:739-746)
                next_id=[L + 1] * P,                 # FilterParticle.next_id (:298)
                used=[0] * P,                        # spare slots in use
                slot_id=[dict() for _ in range(P)])  # spare slot -> feature id
        self.record_ids = (not self._nl_device) if record_ids is None else bool(record_ids)
        self._record_path = int(record_path)
        if self._record_path < 0:
            self._filter.close()
            raise ValueError("record_path must be a number of steps >= 0")
        self._settle_path = max(1, self._record_path // 4) if settle_path is True else int(settle_path or 0)
        if self._settle_path < 0 or (self._settle_path and not self._record_path) or self._settle_path > self._record_path:
            self._filter.close()
            raise ValueError("settle_path=%r: a number of rows in [1, record_path] of a filter that records its path "
                             "(record_path=%d), True, or None" % (settle_path, self._record_path))
        if self._record_path:
            self._filter.path_enable(self._record_path)
        if self._settle_path:
            self._filter.path_trunk_enable(self._settle_path)
        self.Qt = _default_Qt()
        self._domain = {"linear": _lib.PK_WEIGHTS_LINEAR, "log": _lib.PK_WEIGHTS_LOG}[weight_domain]
        if rng not in ("global", "device"):
            raise ValueError("rng must be 'global' or 'device'")
        self._rng = rng
        self._seed = int(seed)
        self._draw = 0
        self._gen = 0
        self._pose_cache = None
        self._probe = None
        self.particles = _ParticleList(self)
        self.last_ids = None
        r = msgs.ros()
        self._publish = (r is not None) if publish_debug is None else bool(publish_debug)
        if r is not None:
            self.aged_particles_pub = r.Publisher('/aged_particles', Odometry, queue_size=1)
            self.resampled_particles_pub = r.Publisher('/resampled_particles', Odometry, queue_size=1)
            self.particle_track_pub = r.Publisher('/particle_track', Odometry, queue_size=1)
        else:
            self.aged_particles_pub = self.resampled_particles_pub = self.particle_track_pub = None
            self._publish = False

    # ------------------------------------------------------------------ views
    def _touch(self):
        self._gen += 1
        self._pose_cache = None
        self._nl_cache = None

    def _nl(self):
        """The new-landmark bookkeeping of every particle as host lists (device mode: one download, kept until the next change)."""
        if not self._nl_device:
            return self._nl_host
        if self._nl_cache is None:
            self._nl_cache = _nl_unpack(*self._filter.grow_download(), L0=self._L0)
        return self._nl_cache

    _hyp = property(lambda self: self._nl()["hyp"])
    _next_id = property(lambda self: self._nl()["next_id"])
    _used = property(lambda self: self._nl()["used"])
    _slot_id = property(lambda self: self._nl()["slot_id"])

    def _nl_particle(self, i):
        """(next_id, readings, spare slot -> id) of particle i."""
        if not self._nl_device:
            h = self._nl_host
            return h["next_id"][i], h["hyp"][i], dict(h["slot_id"][i])
        one = _nl_unpack(*self._filter.grow_download(i, i + 1), L0=self._L0)
        return one["next_id"][0], one["hyp"][0], one["slot_id"][0]

    def _nl_assign(self, hyp, next_id, used, slot_id):
        """Replace the whole bookkeeping (load_state)."""
        if not self._nl_device:
            self._nl_host = dict(hyp=hyp, next_id=next_id, used=used, slot_id=slot_id)
            return
        P = self.num_particles
        _, S, R = self._filter.grow_shape()
        cnt, rd, sid = _nl_pack(hyp, next_id, used, slot_id, self._L0, S, R)
        self._filter.grow_upload(0, P, cnt, rd, sid)
        self._nl_cache = None

    def association_stats(self):
        """Unique association's figures of the last scan (association="unique"; pk_assoc_unique_stats): particles whose
        maximum-likelihood ids claimed some landmark twice, blobs whose id changed, of those the ones matched to another landmark,
        the most passes any particle took.  All zero with association="ml"."""
        with self._lock:
            c = self._filter.assoc_unique_stats()
        return dict(conflicts=int(c[0]), changed=int(c[1]), rematched=int(c[2]), rounds=int(c[3]))

    def readings_dropped(self):
        """Orphaned readings that found the particle's ring full (bookkeeping="device"; the reference's dict grows without
        bound): 0 means the device bookkeeping is the reference's."""
        if not self._nl_device:
            return 0
        return int(self._filter.grow_download(readings=False, slot_ids=False)[0][:, 3].sum())

    def retired(self):
        """(readings, features) retired so far, summed over the particles (reading_max_age / potential_max_idle; (0, 0) without)."""
        if not any(self._retire):
            return 0, 0
        with self._lock:
            c = self._filter.grow_clocks_download()[0]
        return int(c[:, 2].sum()), int(c[:, 3].sum())

    def view_stats(self):
        """With ``view=``: (unchanged spare slots the last retirement pass knew, those of them in view -- the ones that aged --,
        potential features retired, confirmed features retired), summed over the particles (pk_grow_view_stats)."""
        if self._view is None:
            raise ValueError("FastSLAM.view_stats(): this filter was made without view=(half_fov, r_min, r_max)")
        with self._lock:
            return tuple(int(v) for v in self._filter.grow_view_stats())

    def _poses(self):
        if self._pose_cache is None:
            self._pose_cache = self._filter.download_poses()
        return self._pose_cache

    def _particle_view(self, i):
        with self._lock:
            x, y, h, w = self._poses()[i]
            p = FilterParticle(_make_state(x, y, h))
            p.weight = float(w)
            p.Qt = self.Qt
            p._device = self._device
            p.next_id, hyp_i, slot_id = self._nl_particle(i)
            filt, ids, feats, lock = self._filter, self._ids, self._features, self._lock
            if self._grow:
                for rd in hyp_i:
                    b = Blob()
                    b.bearing = rd[4]
                    b.color.r, b.color.g, b.color.b = rd[5], rd[6], rd[7]
                    p.hypothesis_set[rd[0]] = (_make_state(rd[1], rd[2], rd[3]), b)

            def load_all():
                with lock:
                    m, c, k = filt.download_landmarks(i, i + 1)
                full, potential = {}, {}
                for j, id_ in enumerate(ids):
                    f = Feature(mean=m[0, j], covar=c[0, j])
                    f.update_count = int(k[0, j]) & ~_lib.PK_LANDMARK_POTENTIAL
                    f.__immutable__ = bool(feats[j].__immutable__)
                    full[id_] = f
                for slot, id_ in slot_id.items():
                    f = Feature(mean=m[0, slot], covar=c[0, slot])
                    f.update_count = int(k[0, slot]) & ~_lib.PK_LANDMARK_POTENTIAL
                    if int(k[0, slot]) & _lib.PK_LANDMARK_POTENTIAL:
                        potential[-id_] = f  # :685
                    else:
                        full[id_] = f        # promoted (:115-116)
                return full, potential

            p.feature_set = _FeatureSet(lambda: load_all()[0])
            if slot_id:
                p.potential_features = load_all()[1]
            return p

    def _store_particle(self, i, particle):
        """``fs.particles[i] = particle`` (the reference does this at :162): write the pose,
        weight and landmark estimates of a host particle into slot i."""
        with self._lock:
            x, y, h = _state_pose(particle.state)
            self._filter.upload_pose(i, (x, y, h, float(particle.weight)))  # (the other particles' log-weights stay as they are)
            L = len(self._ids)
            if L and all(k in particle.feature_set for k in self._ids):
                fs_ = [particle.feature_set[k] for k in self._ids]
                means = np.array([np.asarray(f.mean, dtype=np.float64) for f in fs_]).reshape(1, L, 5)
                covs = np.array([np.asarray(f.covar, dtype=np.float64) for f in fs_]).reshape(1, L, 25)
                cnts = np.array([int(f.update_count) for f in fs_], dtype=np.int32).reshape(1, L)
                if self._spare:  # the preset landmarks only: the spare slots keep what the filter put there
                    m, c, k = self._filter.download_landmarks(i, i + 1)
                    m[:, :L], k[:, :L] = means, cnts
                    c = c.reshape(1, -1, 25)
                    c[:, :L] = covs
                    means, covs, cnts = m, c, k
                self._filter.upload_landmarks(i, i + 1, means, covs, cnts)
            self._touch()

    def _publish_all(self, pub, poses):
        if not self._publish or pub is None:
            return
        for x, y, h, _w in poses:
            st = _make_state(x, y, h)
            st.header.frame_id = 'odom'
            pub.publish(st)

    # ------------------------------------------------------------------ a12
    def cam_cb(self, ros_view):
        """One filter step (:59-137)."""
        if self._proposal == "measurement":
            return self._cam_cb_proposed(ros_view)
        with self._lock:
            self._motion_update(self.last_control)  # :75-77 (odometry mode: the poses are current up to the last /odom message)
            scan = ros_view.last_sensor_reading  # :82
            observes, ranges = _scan_with_ranges(scan.observes, self._range_noise)
            blobs = _blob_matrix(observes)
            self._filter.set_measurement_noise(self.Qt)
            if ranges is not None and len(blobs) and not np.isnan(ranges).all():
                # the next observe consumes them (pk_scan_ranges); the variance of a range is formed here
                sigma = self._range_noise[0] + self._range_noise[1] * ranges
                self._filter.scan_ranges(ranges, sigma * sigma)
            # :73 weight = 1 (the reset is fused into the observe kernels: pk_observe_fresh; the motion
            # update in between does not read the weights), :84-124 association + EKF + weights
            # (adaptive resampling: no reset -- the weights carry over from a kept step, and a resample leaves them at 1)
            fresh = self._threshold is None
            if self._grow and len(blobs) and not self._nl_device:
                self.last_ids = self._filter.observe(blobs, fresh=fresh, return_ids=True)
                self._touch()
                self._new_landmarks(blobs, self.last_ids)  # :92-95 for every particle's unmatched blobs
            elif self._nl_device and len(blobs):
                # :92-95 on the device, behind the association and the updates (k_new_landmarks)
                self.last_ids = self._filter.observe(blobs, fresh=fresh, return_ids=self.record_ids)
            else:
                self._filter.observe(blobs, fresh=fresh)
            self._touch()
            if self._publish:
                self._publish_all(self.particle_track_pub, self._poses())  # :126-127
            self.low_variance_resample()  # :137
            self._steps_done = getattr(self, "_steps_done", 0) + 1
            if self._nl_device and not getattr(self, "_warned_dropped", False) and self._steps_done % 16 == 0:
                # (the reference's hypothesis_set grows without bound; the device ring holds reading_capacity orphaned
                # readings per particle and counts what it has to drop -- say so once, not only through readings_dropped())
                n = self.readings_dropped()
                if n:
                    import warnings

                    warnings.warn("FastSLAM(new_landmarks=True): %d orphaned readings found their particle's ring full and were dropped "
                                  "(reading_capacity=%d per particle; the reference keeps every reading): later unknown landmarks may not be "
                                  "triangulated -- raise reading_capacity, or use bookkeeping='host'" % (n, self._filter.grow_shape()[2]),
                                  RuntimeWarning, stacklevel=2)
                    self._warned_dropped = True

    def _cam_cb_proposed(self, ros_view):
        """cam_cb with proposal='measurement': the move and the observe are ONE call in which every pose is drawn from the motion
        model conditioned on the scan (pk_propose / pk_propose_odom) -- the same dt bookkeeping, the same draw counter.  Odometry
        mode: the particles move by the change between the odometry pose they were last moved up to and the latest one; no
        change: a plain observe."""
        with self._lock:
            scan = ros_view.last_sensor_reading
            # (without proposal_ranges a (B, 5) scan is refused: no range_noise here)
            observes, ranges = _scan_with_ranges(scan.observes, self._range_noise if self._proposal_ranges else None)
            blobs = _blob_matrix(observes)
            self._filter.set_measurement_noise(self.Qt)
            if ranges is not None and len(blobs) and not np.isnan(ranges).all():
                # the one call below consumes them (pk_scan_ranges, pk_proposal_ranges); the variances are formed as cam_cb forms them
                sigma = self._range_noise[0] + self._range_noise[1] * ranges
                self._filter.scan_ranges(ranges, sigma * sigma)
            fresh = self._threshold is None
            want = self._proposal_ids
            z = None
            if self._motion == "twist":
                dt = msgs.now() - self.last_update
                v, w = float(self.last_control.linear.x), float(self.last_control.angular.z)
                z = self._noise(self.num_particles)
                ids = self._filter.propose(v, w, dt.to_sec(), blobs, z=z, seed=self._seed, draw=self._draw, fresh=fresh, return_ids=want)
                self._draw += 1
                self.last_update = self.last_update + dt
            else:
                self._motion_update(self.last_control)  # (records the control and its time, moves nothing)
                prev, now = self._odom_applied, self._odom_prev
                delta = None if prev is None or now is None else _lib.odom_delta(prev, now, self._odom_min_trans)
                self._odom_applied = now
                if delta is None or _odom.is_zero(delta):
                    ids = self._filter.observe(blobs, fresh=fresh, return_ids=want)
                else:
                    z = self._noise(self.num_particles)
                    ids = self._filter.propose_odom(delta, self._odom_alphas, blobs, z=z, seed=self._seed, draw=self._draw, fresh=fresh,
                                                    return_ids=want)
                    self._draw += 1
            if want:
                self.last_ids = ids
            self._touch()
            if self._publish:
                self._publish_all(self.particle_track_pub, self._poses())
            self.low_variance_resample()

    def _new_landmarks(self, blobs, ids):
        """add_hypothesis (:546-564) for every unmatched blob of every particle, in scan order, with the working pairing
        rule (class docstring).  New potential features are written into the particle's next spare slot."""
        poses = self._poses()
        scratch = FilterParticle()
        tri = self._landmark_init == "triangulated"
        sin_min, q00 = math.sin(self._min_parallax), float(np.asarray(self.Qt, dtype=np.float64)[0, 0])
        for i in np.nonzero((ids == 0).any(axis=1))[0]:
            i = int(i)
            x, y, h = float(poses[i, 0]), float(poses[i, 1]), float(poses[i, 2])
            fresh = []
            for b in np.nonzero(ids[i] == 0)[0]:
                z = blobs[b]
                best, best_d = None, float('inf')
                for rd in self._hyp[i]:  # find_nearest_reading :566-590 over the stored readings
                    if not scratch.ray_intersect(rd[1], rd[2], rd[4] + rd[3], x, y, float(z[0]) + h):  # :592-609
                        continue
                    if tri and not (abs(scratch._ray_determinant(rd[4] + rd[3], float(z[0]) + h)) >= sin_min):  # the parallax gate
                        continue
                    d = math.sqrt(math.pow(rd[5] - z[1], 2) + math.pow(rd[6] - z[2], 2) + math.pow(rd[7] - z[3], 2))
                    if d < best_d:
                        best, best_d = rd, d
                xy = None
                if best is not None and best_d < self._pair_threshold and self._used[i] + len(fresh) < self._spare:
                    xy = scratch._cross_lines(best[1], best[2], best[3] + best[4], x, y, h + float(z[0]))  # :688-737
                if xy is not None:  # add_new_feature :656-686
                    slot = self._L0 + self._used[i] + len(fresh)
                    pos = None
                    if tri:
                        pos = scratch._triangulated_covariance(best[1], best[2], best[3] + best[4], x, y, h + float(z[0]), xy[0], xy[1], q00)
                    fresh.append((slot, (xy[0], xy[1], (best[5] + z[1]) / 2, (best[6] + z[2]) / 2, (best[7] + z[3]) / 2), pos))
                    self._slot_id[i][slot] = self._next_id[i]
                else:  # add_orphaned_reading :739-746
                    self._hyp[i].append((self._next_id[i], x, y, h, float(z[0]), float(z[1]), float(z[2]), float(z[3])))
                self._next_id[i] += 1
            if fresh:
                m, c, k = self._filter.download_landmarks(i, i + 1)
                for slot, mean, pos in fresh:
                    m[0, slot] = mean
                    c[0, slot] = np.identity(5)
                    if pos is not None:
                        c[0, slot, 0, 0], c[0, slot, 0, 1], c[0, slot, 1, 0], c[0, slot, 1, 1] = pos[0], pos[1], pos[1], pos[2]
                    k[0, slot] = _lib.PK_LANDMARK_POTENTIAL  # update_count 0, potential
                self._filter.upload_landmarks(i, i + 1, m, c.reshape(1, -1, 25), k)
                self._used[i] += len(fresh)

    def odom_motion_update(self, odom):
        """:140-146, empty in the reference.  motion="odometry": move every particle by the change between the last odometry
        message's pose and this one's (pk_odom_delta, pk_motion_odom); the first message only stores its pose.  A robot that
        stood still (a delta of exactly zero) launches nothing and consumes no draw.  motion="twist": nothing, as the reference."""
        if self._motion != "odometry":
            return
        now = _odom.check_pose(_state_pose(odom))  # (a message that is not finite: ValueError, nothing stored, nothing moved)
        with self._lock:
            prev = self._odom_prev
            delta = None if prev is None else _lib.odom_delta(prev, now, self._odom_min_trans)
            self._odom_prev = now  # (only once the delta was formed: a refused message leaves the stored pose as it was)
            if self._proposal == "measurement":  # the message is stored: cam_cb moves by it, conditioned on its scan
                if self._odom_applied is None:
                    self._odom_applied = now
                return
            if delta is None or _odom.is_zero(delta):
                return
            self._filter.motion_odom(delta, self._odom_alphas, z=self._noise(self.num_particles), seed=self._seed, draw=self._draw)
            self._draw += 1
            self._touch()

    # ------------------------------------------------------------------ a2
    def _noise(self, n):
        if self._rng == "global":
            # numpy.random.normal(0, s, 1) x 3 per particle, particle-major (:185-193), is the
            # same stream as one standard_normal(3 P) call scaled by s (legacy loc + scale*gauss)
            return np.random.standard_normal((n, 3))
        return None

    def _motion_update(self, new_twist):
        dt = msgs.now() - self.last_update  # :158
        if self._motion == "twist":
            v = float(self.last_control.linear.x)  # moves with the PREVIOUS control (:163)
            w = float(self.last_control.angular.z)
            self._filter.motion(v, w, dt.to_sec(), z=self._noise(self.num_particles), seed=self._seed, draw=self._draw)
            self._draw += 1
            self._touch()
        # (motion="odometry": the control and its time are recorded, the particles move by odom_motion_update alone)
        self.last_update = self.last_update + dt  # :165
        self.last_control = new_twist  # :166

    def motion_update(self, new_twist):
        with self._lock:
            self._motion_update(new_twist)

    def motion_model(self, particle, twist, dt):
        """Move ONE particle (:168-208) and return the moved copy.  Runs the same kernel on a
        one-particle filter."""
        dt = dt.to_sec()
        x, y, h = _state_pose(particle.state)
        with self._lock:
            if self._probe is None:  # one one-particle filter per FastSLAM, made on first use (a stream + buffers: ~ms to create)
                self._probe = _lib.DeviceFilter(1, 0, device=self._device)
            f = self._probe
            f.upload_poses(np.array([[x, y, h, 1.0]]))
            z = self._noise(1)
            f.motion(float(twist.linear.x), float(twist.angular.z), dt, z=z, seed=self._seed, draw=self._draw)
            self._draw += 1
            nx, ny, nh, _ = f.download_poses()[0]
        new_particle = _copy.deepcopy(particle)
        new_particle.state = _copy.deepcopy(particle.state)
        new_particle.state.pose.pose.position.x = nx
        new_particle.state.pose.pose.position.y = ny
        new_particle.state.pose.pose.orientation = heading_to_quaternion(nh)
        return new_particle

    # ------------------------------------------------------------------ a13
    def low_variance_resample(self):
        with self._lock:
            if self._publish:
                self._publish_all(self.aged_particles_pub, self._poses())  # :237
            u = _pyrandom.random()  # :226
            host_nl = self._grow and not self._nl_device
            want = self._publish or host_nl or (self._grow and self.record_ids)
            if self._threshold is None:
                self.last_ancestors = self._filter.resample(u, domain=self._domain, return_ancestors=want)
            else:  # decided on the device; a kept step's ancestors are the identity, so the gather below holds either way
                self.last_ancestors = self._filter.resample_adaptive(u, self._threshold, domain=self._domain, return_ancestors=want)
            if host_nl:  # (device mode: pk_resample gathers the bookkeeping with the particles)
                anc = [int(a) for a in self.last_ancestors]
                h = self._nl_host
                self._nl_host = dict(hyp=[list(h["hyp"][a]) for a in anc], next_id=[h["next_id"][a] for a in anc],
                                     used=[h["used"][a] for a in anc], slot_id=[dict(h["slot_id"][a]) for a in anc])
            self._touch()
            if self._publish:
                self._publish_all(self.resampled_particles_pub, self._poses())  # :242

    # ------------------------------------------------------------------ a14
    def summary(self):
        """(x, y, heading): the particles' mean pose (:254-276) -- by their weights on a filter that resamples adaptively."""
        with self._lock:
            if self._threshold is not None:
                return self._filter.summary_weighted(self._domain).pose()
            return self._filter.summary()

    def pose_summary(self):
        """The pose estimate by the particles' weights (``adaptive.PoseSummary``: mean, spread, n_eff) of a filter that resamples
        adaptively.  (One that resamples behind every scan keeps the weights its particles were chosen by until the next scan
        resets them: weighting the chosen particles by them again would count them twice -- summary() is its estimate.)"""
        if self._threshold is None:
            raise ValueError("pose_summary: this filter resamples at every step (FastSLAM(..., resample_threshold=theta)); its estimate is summary()")
        with self._lock:
            return self._filter.summary_weighted(self._domain)

    def resample_stats(self):
        """What the last step's gate decided and how many steps resampled so far (``adaptive.ResampleStats``)."""
        if self._threshold is None:
            raise ValueError("resample_stats: this filter resamples at every step (FastSLAM(..., resample_threshold=theta))")
        with self._lock:
            return self._filter.resample_stats()

    def map_summary(self, weighting=None):
        """The map estimate, reduced over the particles on the device (``mapsum.MapSummary``; the sibling of summary(),
        prkt_core_v2.py:254-276, which stops at the pose).  weighting "uniform": every particle counts once, as in summary() --
        behind a resample the population is the estimate; "weights": by the particles' weights, for use between an observe
        and a resample -- the default on a filter that resamples adaptively, whose weights carry over.  A growing filter's
        spare landmarks are NaN rows (``as_features()`` leaves them out)."""
        if weighting is None:
            weighting = "uniform" if self._threshold is None else "weights"
        code = mapsum.weighting_code(weighting)
        with self._lock:
            return self._filter.map_summary(code)

    def discovered_landmarks(self, weighting=None, reference=None, radius=3.0, colour_radius=None):
        """The estimate of the landmarks the filter DISCOVERED (new_landmarks=True), which map_summary() leaves NaN: spare slot
        j of one particle and of another need not hold the same feature, so the features of one reference particle (None: the
        most likely one, best_particle()) are matched in every particle by position and colour and reduced over the particles
        that hold them, on the device (``mapsum.DiscoveredMap``: per feature the mean, the covariances, the share of the
        population that holds it).  weighting as for map_summary().  A slot matches inside ``radius`` (3.0: three standard
        deviations of the identity position covariance a new feature is born with) and ``colour_radius`` (None: the filter's
        pair_threshold, the colour distance under which two readings already count as one landmark); the nearest wins.  The
        matches are taken per feature, NOT one-to-one: keep ``radius`` below half the smallest landmark separation."""
        if not self._grow:
            raise ValueError("discovered_landmarks: this filter discovers no landmarks (FastSLAM(..., new_landmarks=True, spare_landmarks=S))")
        if not self._nl_device:
            raise ValueError("discovered_landmarks: the match reads the bookkeeping on the device (bookkeeping='device' and spare_landmarks > 0)")
        if weighting is None:
            weighting = "uniform" if self._threshold is None else "weights"
        code = mapsum.weighting_code(weighting)
        kappa = self._pair_threshold if colour_radius is None else float(colour_radius)
        with self._lock:
            return self._filter.map_discovered(float(radius), kappa, code, reference)

    def _need_path(self, who):
        if not self._record_path:
            raise ValueError("%s: this filter does not record its path (FastSLAM(..., record_path=T))" % who)

    def path_summary(self, weighting="uniform"):
        """The path estimate (``path.PathSummary``): per step of the ring, oldest first, and for the current generation last, the
        mean pose over the lineages of the current particles, their spread, and how many distinct ancestors they still have
        there -- the trajectory the filter NOW believes in, not the string of per-step summary() values.  weighting "uniform"
        (the default, on every filter): every current particle counts once; "weights": by the particles' weights in the filter's
        weight domain (``path.WeightedPathSummary``: mean, spread and n_eff), the estimate between an observe and a resample of a
        filter that resamples adaptively."""
        self._need_path("path_summary")
        if weighting not in ("uniform", "weights"):
            raise ValueError('path_summary: weighting must be "uniform" or "weights", not %r' % (weighting,))
        with self._lock:
            if weighting == "weights":
                return self._filter.path_summary_weighted(self._domain)
            return self._filter.path_summary()

    def full_path(self, weighting="uniform"):
        """The path of the whole run (``path.FullPath``): the trunk's settled rows (FastSLAM(..., settle_path=E)), then
        ``path_summary(weighting)``'s rows of the ring and of the current generation -- steps first_step .. recorded without a
        gap.  A trunk row is ``final`` where every particle that was current when it was settled descended from one ancestor; a
        ring row where the uniform summary reports one survivor.  Under "weights" the ring's rows are all reported not final:
        the weighted summary counts no ancestors, and a row with one WEIGHTED lineage but several lineages overall is not final
        -- this errs on the safe side.  Without settle_path it is path_summary in FullPath's form."""
        self._need_path("full_path")
        with self._lock:
            summary = self.path_summary(weighting)
            ring_final = summary.survivors == 1 if weighting == "uniform" else np.zeros(summary.mean.shape[0], dtype=bool)
            trunk = None
            if self._settle_path:
                trunk = self._filter.path_trunk_summary() + (self._filter.path_trunk_shape()[1],)
            return _path.FullPath.assemble(trunk, summary, ring_final)

    def best_particle(self):
        """The index of the particle with the largest weight (the lowest one among equals)."""
        with self._lock:
            return self._filter.best_particle()[0]

    def best_path(self):
        """The path of the most likely particle, array (held + 1, 3) of (x, y, heading): ``particle_paths([best_particle()])[0]``."""
        self._need_path("best_path")
        with self._lock:
            return self._filter.path_trace([self._filter.best_particle()[0]])[0]

    def particle_paths(self, indices):
        """The paths of the listed current particles, array (len, held + 1, 3) of (x, y, heading); the last row is particles[i]."""
        self._need_path("particle_paths")
        with self._lock:
            return self._filter.path_trace(indices)

    # ------------------------------------------------------------------ snapshot / restore
    def save_state(self, path):
        """Whole filter state -> .npz (poses, weights, every particle's landmark means /
        covariances / update counts, Qt, controls).  The reference has no checkpointing
        (SURVEY section 5); this is the state round trip tests and long runs want."""
        with self._lock:
            poses = self._filter.download_poses()
            m, c, k = self._filter.download_landmarks()
            extra = {}
            if self._nl_device:
                extra = _nl_snapshot_arrays(*self._filter.grow_download(), L0=self._L0)
                if any(self._retire):  # the clocks of the retirement rule, whole (rows beyond what a particle holds: zeroed)
                    kc, sc, se, si, now = self._filter.grow_clocks_download()
                    sc[np.arange(sc.shape[1])[None, :] >= kc[:, :1]] = 0
                    se[np.arange(se.shape[1])[None, :] >= kc[:, 1:2]] = 0
                    si[np.arange(si.shape[1])[None, :] >= kc[:, 1:2]] = 0
                    extra.update(nl_clock_counters=kc,nl_clock_scan=sc, nl_clock_seen=se, nl_clock_idle=si, nl_clock_now=np.uint32(now))
            elif self._grow:
                extra = _nl_snapshot(self._nl())
            if self._grow:
                extra.update(landmark_init=np.array(self._landmark_init), min_parallax=np.float64(self._min_parallax))
            if self._grow_ranges:  # (off: no field -- a snapshot without it restores as off)
                extra["grow_ranges"] = np.bool_(True)
            if self._threshold is not None:  # the weights carry over: bit for bit, not through exp and log
                extra["log_weights"] = self._filter.download_log_weights()
            if self._record_path:
                extra["path_poses"], extra["path_ancestors"] = self._filter.path_download()
                extra["path_recorded"] = np.int64(self._filter.path_shape()[2])
            if self._motion == "odometry" and self._odom_prev is not None:
                extra["odom_prev"] = np.array(self._odom_prev, dtype=np.float64)
            if self._settle_path:
                extra["path_trunk_rows"] = self._filter.path_trunk_download()
                extra["path_trunk_first"] = np.int64(self._filter.path_trunk_shape()[1])
            np.savez_compressed(
                path, poses=poses, means=m, covs=c, counts=k, Qt=np.asarray(self.Qt, dtype=np.float64),
                immutable=np.array([bool(f.__immutable__) for f in self._features], dtype=np.uint8),
                last_control=np.array([float(self.last_control.linear.x), float(self.last_control.angular.z)]),
                last_update=float(self.last_update.to_sec()), draw=self._draw,
                measurement_model=np.array(self._model), **extra)

    def load_state(self, path):
        with self._lock:
            d = np.load(path, allow_pickle=False)  # numeric arrays only: loading a snapshot never runs code
            P, L = self.num_particles, self._L0 + self._spare
            if d["poses"].shape != (P, 4) or d["means"].shape != (P, L, 5):
                raise ValueError("snapshot is for %s particles x %s landmarks, this filter has %d x %d"
                                 % (d["poses"].shape[0], d["means"].shape[1], P, L))
            # (a snapshot from before the field: the reference model)
            model = str(d["measurement_model"]) if "measurement_model" in d.files else "reference"
            if model != self._model:
                raise ValueError("snapshot: taken with measurement_model=%r, this filter runs %r -- the states of the two models "
                                 "do not continue each other" % (model, self._model))
            if self._grow and "nl_offsets" not in d.files:
                # (snapshots of before round 3 kept the bookkeeping as a pickled object array "new_landmarks": not read any
                # more -- and a growing filter whose maps are replaced while its bookkeeping stays is inconsistent)
                raise ValueError("snapshot: no new-landmark bookkeeping (nl_* arrays) for a filter with new_landmarks=True%s"
                                 % ("; it was written in the old pickled format" if "new_landmarks" in d.files else ""))
            have_nl = "nl_offsets" in d.files and self._grow
            if self._grow:  # (a snapshot from before the fields: the reference's rule)
                init = _check_landmark_init(str(d["landmark_init"]) if "landmark_init" in d.files else "reference",
                                            float(d["min_parallax"]) if "min_parallax" in d.files else self._min_parallax, True, "snapshot")
            ranged = bool(d["grow_ranges"]) if "grow_ranges" in d.files else False
            if ranged and not (self._nl_device and self._range_noise is not None and (self._proposal == "motion" or self._proposal_grow)):
                raise ValueError("snapshot: taken with grow_ranges=True, which needs this filter's range_noise=(sigma0, sigma1), "
                                 "new_landmarks=True with spare_landmarks > 0, bookkeeping='device' and proposal='motion'")
            have_path = self._record_path and "path_ancestors" in d.files
            if have_path:
                n = d["path_ancestors"].shape[0]
                if d["path_ancestors"].shape != (n, P) or d["path_poses"].shape != (n, P, 3) or n > self._record_path:
                    raise ValueError("snapshot: a path of %s x %s does not fit this filter's ring of %d steps x %d particles"
                                     % (d["path_ancestors"].shape[0], d["path_ancestors"].shape[1:], self._record_path, P))
            have_trunk = self._settle_path and "path_trunk_rows" in d.files
            if have_trunk:
                rows = d["path_trunk_rows"]
                if rows.ndim != 2 or rows.shape[1] != _path.TRUNK_RES or int(d["path_trunk_first"]) < 0:
                    raise ValueError("snapshot: path_trunk_rows must be (n, %d) from a step >= 0" % _path.TRUNK_RES)
                if rows.shape[0] and not (np.all(rows[:, 8] >= 0) and np.all(rows[:, 8] <= rows[:, 9]) and np.all(rows[:, 9] < P)
                                          and np.all(rows[:, 8:10] == np.floor(rows[:, 8:10]))):
                    raise ValueError("snapshot: the trunk's ancestors are not lineage indices of %d particles" % P)
                n_ring = d["path_ancestors"].shape[0] if have_path else 0
                end = int(d["path_recorded"]) - n_ring if have_path else int(d["path_trunk_first"]) + rows.shape[0]
                if int(d["path_trunk_first"]) + rows.shape[0] != end:
                    raise ValueError("snapshot: a trunk of steps [%d, %d) does not meet a ring that begins at step %d"
                                     % (int(d["path_trunk_first"]), int(d["path_trunk_first"]) + rows.shape[0], end))
            have_logw = self._threshold is not None and "log_weights" in d.files
            if have_logw and (d["log_weights"].shape != (P,) or not np.all(d["log_weights"] < np.inf)):
                raise ValueError("snapshot: log_weights must be %d numbers below +inf" % P)
            have_odom = self._motion == "odometry" and "odom_prev" in d.files
            if have_odom and (d["odom_prev"].shape != (3,) or not np.all(np.isfinite(d["odom_prev"]))):
                raise ValueError("snapshot: odom_prev must be a finite pose (x, y, heading)")
            if have_nl:  # everything is checked before anything is assigned
                _nl_check_snapshot(d, P, self._L0, L, self._spare, self._filter.grow_shape()[2] if self._nl_device else None)
            # (a snapshot without the clocks, or a filter that retires nothing: pk_grow_upload restarts them / they are not read)
            have_clocks = have_nl and self._nl_device and any(self._retire) and "nl_clock_counters" in d.files
            if have_clocks:
                _, S, R = self._filter.grow_shape()
                kc = d["nl_clock_counters"]
                if (kc.shape != (P, 4) or d["nl_clock_scan"].shape != (P, R) or d["nl_clock_seen"].shape != (P, S)
                        or d["nl_clock_idle"].shape != (P, S) or (kc < 0).any()
                        or (kc[:, 0] > np.diff(d["nl_offsets"])).any() or (kc[:, 1] > d["nl_used"]).any()):
                    raise ValueError("snapshot: the retirement clocks (nl_clock_*) do not fit this filter's %d particles, rings of %d "
                                     "readings and %d spare slots, or cover more than a particle holds" % (P, R, S))

            self._filter.upload_poses(d["poses"])
            if have_logw:  # (a snapshot without them: log(weight), as upload_poses took it)
                self._filter.upload_log_weights(d["log_weights"])
            if L:
                self._filter.upload_landmarks(0, P, d["means"], d["covs"].reshape(P, L, 25), d["counts"])
            self.Qt = d["Qt"].copy()
            self.last_control.linear.x = float(d["last_control"][0])
            self.last_control.angular.z = float(d["last_control"][1])
            self._draw = int(d["draw"])
            if self._motion == "odometry":  # (a snapshot without the pose: the next message is the first)
                self._odom_prev = tuple(float(v) for v in d["odom_prev"]) if have_odom else None
            if self._grow:
                self._landmark_init, self._min_parallax = init
                if self._nl_device:
                    self._filter.grow_init(*init)
                    self._grow_ranges = ranged
                    self._filter.grow_ranges(ranged)
            if have_nl and self._nl_device:
                _, S, R = self._filter.grow_shape()
                self._filter.grow_upload(0, P, *_nl_arrays_from_snapshot(d, P, self._L0, S, R))
                if have_clocks:
                    self._filter.grow_clocks_upload(0, P, d["nl_clock_counters"], d["nl_clock_scan"], d["nl_clock_seen"],
                                                    d["nl_clock_idle"], int(d["nl_clock_now"]))
            elif have_nl:
                self._nl_assign(*_nl_restore(d, P))
            if have_trunk:  # (behind upload_poses, ahead of the ring; a snapshot without it: the trunk restarts where the ring begins)
                self._filter.path_trunk_upload(d["path_trunk_rows"], int(d["path_trunk_first"]))
            if have_path:  # (behind upload_poses, which empties the ring; a snapshot without a path leaves it empty)
                self._filter.path_upload(d["path_poses"], d["path_ancestors"], int(d["path_recorded"]))
            self._touch()

    def close(self):
        if self._probe is not None:
            self._probe.close()
            self._probe = None
        self._filter.close()

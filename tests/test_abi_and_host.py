"""CPU: the C-ABI library loads without a GPU, exports every symbol the header declares,
refuses to compute without a device (no CPU fallback), and its host-side RNG
reproductions match NumPy / CPython bit for bit."""
import ctypes
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "parakeet_slam.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_declares_expected_entry_points():
    names = declared_functions()
    for must in ("pk_create", "pk_destroy", "pk_upload_map", "pk_motion", "pk_observe", "pk_observe_fresh", "pk_stage_scan", "pk_observe_staged", "pk_observe_route", "pk_associate",
                 "pk_resample", "pk_summary", "pk_step", "pk_probe", "pk_timings", "pk_download_poses",
                 "pk_download_landmarks", "pk_rng_standard_normal", "pk_shard_block_totals"):
        assert must in names


def test_library_exports_every_declared_symbol(lib):
    so = lib.load()
    for name in declared_functions():
        assert hasattr(so, name), "libparakeet_slam.so does not export %s" % name


def test_binding_covers_every_declared_symbol(lib):
    assert sorted(lib.SIGNATURES) == declared_functions()


def test_abi_version_and_status_strings(lib):
    so = lib.load()
    assert so.pk_abi_version() == lib.PK_ABI_VERSION
    assert so.pk_status_string(0) == b"ok"
    assert b"unsupported" in so.pk_status_string(lib.PK_ERR_UNSUPPORTED)


def _no_gpu(lib):
    return lib.load().pk_device_count() == 0


def test_no_cpu_fallback_without_device(lib):
    if not _no_gpu(lib):
        pytest.skip("a HIP device is visible")
    with pytest.raises(lib.PkError) as ei:
        lib.DeviceFilter(8, 2)
    assert ei.value.status == lib.PK_ERR_HIP and "no CPU fallback" in str(ei.value)
    with pytest.raises(lib.PkError):
        lib.probe((0, 0, 0), (1, 0, 0, 0, 0), np.identity(5), (0, 0, 0, 0))
    import parakeet_slam_amd as pk

    with pytest.raises(lib.PkError):
        pk.FastSLAM([pk.Feature()])


def test_missing_library_is_loud(lib, tmp_path, monkeypatch):
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(OSError) as ei:
        lib.load()
    assert "no CPU fallback" in str(ei.value)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "parakeet_slam_amd")
    for dirpath, _dirs, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                text = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), fn
                assert "fastslam_oracle" not in text, fn


@pytest.mark.parametrize("seed", [0, 1, 7, 12345, 2**32 - 1])
def test_numpy_legacy_normal_stream(lib, seed):
    # prkt_core_v2.py:27,185-193 draws numpy.random.normal(0, s, 1): legacy MT19937 + polar method
    got = lib.HostRng(seed, "numpy").standard_normal(4001)
    ref = np.random.RandomState(seed).standard_normal(4001)
    assert np.array_equal(got, ref)
    np.random.seed(seed)
    glob = np.array([np.random.normal(0, 1.0, 1)[0] for _ in range(50)])
    assert np.array_equal(got[:50], glob)


@pytest.mark.parametrize("seed", [0, 1, 7, 12345, 2**32 - 1])
def test_python_random_stream(lib, seed):
    # prkt_core_v2.py:28,226 random.random()
    got = lib.HostRng(seed, "python").random(3000)
    r = random.Random(seed)
    assert np.array_equal(got, np.array([r.random() for _ in range(3000)]))


def test_rng_interleaves_like_numpy(lib):
    # the cached second variate of the polar method survives across calls
    r = lib.HostRng(99, "numpy")
    a = np.concatenate([r.standard_normal(3), r.standard_normal(4), r.standard_normal(1)])
    assert np.array_equal(a, np.random.RandomState(99).standard_normal(8))


def test_reference_unavailable_is_only_a_skip():
    # nothing in tests/ may depend on the reference tree at run time: the cross-check on fresh
    # random inputs reads the reference's recorded answers (tests/golden/reference_live.npz)
    needle = "/root/" + "reference"
    for fn in os.listdir(os.path.join(ROOT, "tests")):
        if fn.endswith(".py"):
            assert needle not in open(os.path.join(ROOT, "tests", fn)).read(), fn


# ---- f4: the reference's own unit tests of the new-landmark geometry (test_prkt_ros2.py:228-381), restated on the
# facade's host methods (prkt_core_v2.py:546-746); no GPU involved
def _reading(pk, x=0.0, y=0.0, heading=None, bearing=0.0, rgb=(0, 0, 0)):
    st = pk.msgs.Odometry()
    st.pose.pose.position.x, st.pose.pose.position.y = x, y
    if heading is not None:
        st.pose.pose.orientation = pk.msgs.heading_to_quaternion(heading)
    b = pk.msgs.Blob()
    b.bearing = bearing
    b.color.r, b.color.g, b.color.b = rgb
    return st, b


def test_find_nearest_reading_reference_test():
    # test_prkt_ros2.py:228-274
    import parakeet_slam_amd as pk

    p = pk.FilterParticle()
    p.potential_features[-1] = _reading(pk, bearing=.1)
    q = _reading(pk, y=1, bearing=-.1)
    assert p.find_nearest_reading(*q) == -1
    p.potential_features[-3] = _reading(pk, y=1, bearing=-.1)  # parallel to the query
    assert p.find_nearest_reading(*q) == -1
    p.potential_features[-4] = _reading(pk, bearing=.1, rgb=(255, 255, 255))  # wrong colour
    assert p.find_nearest_reading(*q) == -1
    p.potential_features[-5] = p.potential_features[-4]
    assert p.find_nearest_reading(*q) == -1
    assert pk.FilterParticle().find_nearest_reading(*q) == 0  # nothing stored: :576


def test_reading_distance_function_reference_test():
    # test_prkt_ros2.py:276-311
    import parakeet_slam_amd as pk

    p = pk.FilterParticle()
    a = _reading(pk)
    assert p.reading_distance_function(*a, *_reading(pk, y=1)) == float("inf")               # parallel
    assert p.reading_distance_function(*a, *_reading(pk, y=1, bearing=1.0)) == float("inf")  # diverging
    assert p.reading_distance_function(*a, *_reading(pk, y=1, bearing=-1.0)) == 0.0
    assert p.reading_distance_function(*a, *_reading(pk, y=1, bearing=-1.0, rgb=(5, 0, 0))) == 5.0


def test_ray_intersect_and_cross_readings_reference_tests():
    # test_prkt_ros2.py:313-346, :352-370
    import parakeet_slam_amd as pk

    p = pk.FilterParticle()
    assert p.ray_intersect(0.0, 0.0, 0.0, 1.0, 0.0, math.pi / 2.0)
    assert p.ray_intersect(0.0, 0.0, math.pi / 4, 1.0, 0.0, 3 * math.pi / 4)
    assert not p.ray_intersect(0.0, 0.0, math.pi / 4, -1.0, 0.0, 3 * math.pi / 4)
    old = _reading(pk)
    got = p.cross_readings(old, _reading(pk, heading=math.pi / 2))
    assert got is not None and got[0] == 0.0 and got[1] == 0.0
    assert p.cross_readings(old, _reading(pk, y=-1.0, heading=0.0)) is None


def test_add_hypothesis_files_orphans_and_add_new_feature_triangulates():
    # :546-564 (always the orphan branch), :656-686
    import parakeet_slam_amd as pk

    p = pk.FilterParticle()
    p.add_hypothesis(*_reading(pk, bearing=0.0, rgb=(10, 20, 30)))
    p.add_hypothesis(*_reading(pk, y=1, bearing=-1.0))
    assert sorted(p.hypothesis_set) == [1, 2] and p.next_id == 3 and not p.potential_features
    p.add_new_feature(1, *_reading(pk, x=2.0, y=-2.0, heading=math.pi / 2, rgb=(30, 40, 50)))
    f = p.potential_features[-3]
    assert p.next_id == 4 and np.allclose(f.mean, [2.0, 0.0, 20, 30, 40], atol=1e-12) and np.array_equal(f.covar, np.identity(5))
    assert p.get_feature_by_id(-3) is f

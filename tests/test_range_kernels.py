"""Host: the built library holds the kernel instances of range-bearing scans (pk_scan_ranges) -- k_observe_range in both shapes,
k_assoc_grid_range in its four, k_assoc_brute_range and the two probe kernels -- and their code-object metadata, read as
test_kernel_resources.py reads it, says what DESIGN.md section 4 says: no scratch, no register spilled to memory."""
import os

import pytest

from test_kernel_resources import READELF, code_object_kernels

INSTANCES = {
    "k_observe_rangeILb1ELi2EE": 1, "k_observe_rangeILb0ELi1EE": 1,
    "k_assoc_grid_rangeILi256ELb1EE": 1, "k_assoc_grid_rangeILi256ELb0EE": 1, "k_assoc_grid_rangeILi512ELb1EE": 1,
    "k_assoc_grid_rangeILi512ELb0EE": 1, "19k_assoc_brute_rangeE": 1, "k_probe_rangeILi0EE": 1, "k_probe_rangeILi1EE": 1,
}


def test_the_library_holds_the_range_instances_without_scratch_or_spills():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from parakeet_slam_amd import build

    ks = code_object_kernels(build.build(verbose=False))
    for needle, n in INSTANCES.items():
        found = [k for k in ks if needle in k["symbol"]]
        assert len(found) == n, (needle, sorted(k["symbol"] for k in ks if "range" in k["symbol"]))
        for k in found:
            assert int(k["private_segment_fixed_size"]) == 0, k
            assert int(k["vgpr_spill_count"]) == 0, k
            assert int(k["vgpr_count"]) <= 256, k  # (256 lanes a workgroup: one wave per SIMD can hold 512)
            print(k["symbol"], "VGPRs", k["vgpr_count"], "SGPRs parked in VGPR lanes", k["sgpr_spill_count"], "static LDS", k["group_segment_fixed_size"])
    # the instances they stand beside keep their names
    names = " ".join(k["symbol"] for k in ks)
    for needle in ("k_observe_bearingILb1ELi2EE", "k_observe_bearingILb0ELi1EE", "k_assoc_grid_bearingILi256ELb1EE", "21k_assoc_brute_bearingE"):
        assert needle in names, needle

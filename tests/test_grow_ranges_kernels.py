"""Host: the built library holds the two ranged instances of the new-landmark bookkeeping kernel -- k_new_landmarks_ranged and
k_new_landmarks_tri_ranged (pk_grow_ranges) -- exactly once each, and their code-object metadata, read as test_grow_init_kernels.py
reads it, says what DESIGN.md section 9 says of this kernel family: no scratch, nothing spilled, no static LDS, and registers for
three waves per SIMD (at most 168 VGPRs of 512)."""
import os

import pytest

from test_kernel_resources import READELF, code_object_kernels


def test_the_library_holds_both_ranged_bookkeeping_kernels_without_scratch_or_lds():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from parakeet_slam_amd import build

    ks = {k["symbol"]: k for k in code_object_kernels(build.build(verbose=False))}
    ranged = [k for s, k in ks.items() if "22k_new_landmarks_rangedE" in s]
    tri = [k for s, k in ks.items() if "26k_new_landmarks_tri_rangedE" in s]
    assert len(ranged) == 1 and len(tri) == 1, sorted(s for s in ks if "new_landmarks" in s)
    for k in ranged + tri:
        print(k["symbol"], "vgprs", k["vgpr_count"], "sgprs", k.get("sgpr_count"))
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_count"]) <= 168, k

"""Host: the built library holds both instances of the new-landmark bookkeeping kernel -- k_new_landmarks (the reference's rule) and
k_new_landmarks_tri (pk_grow_init, PK_GROW_INIT_TRIANGULATED) -- and their code-object metadata, read as test_kernel_resources.py
reads it, says what DESIGN.md section 9 says: no scratch, nothing spilled, no static LDS, and registers for three waves per SIMD
(at most 168 VGPRs of 512; one wave per particle, four particles a block)."""
import os

import pytest

from test_kernel_resources import READELF, code_object_kernels


def test_the_library_holds_both_bookkeeping_kernels_without_scratch_or_lds():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from parakeet_slam_amd import build

    ks = {k["symbol"]: k for k in code_object_kernels(build.build(verbose=False))}
    plain = [k for s, k in ks.items() if "15k_new_landmarksE" in s]
    tri = [k for s, k in ks.items() if "19k_new_landmarks_triE" in s]
    assert len(plain) == 1 and len(tri) == 1, sorted(s for s in ks if "new_landmarks" in s)
    for k in plain + tri:
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_count"]) <= 168, k

"""CPU: the table-mode instances of k_step_pub ("The colour table") as the code objects describe them: no
scratch, one 512-lane workgroup per CU (<= 256 VGPRs), the same static LDS as the plain instances (the publish table's capacity is
what is left of 160 KB), and symbols that parakeet_slam_amd.codeobj files under the plain instance's name."""
import os

import pytest

from test_kernel_resources import READELF, code_object_kernels


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from parakeet_slam_amd import build

    return {k["symbol"].replace(".kd", ""): k for k in code_object_kernels(build.build(verbose=False))}


@pytest.mark.parametrize("np_", [1, 2])
def test_table_mode_instances_fit_one_workgroup_per_cu_without_scratch(kernels, np_):
    plain = kernels["_ZN2pk10k_step_pubILi%dELi512EEEvNS_7PubArgsE" % np_]
    tab = kernels["_ZN2pk10k_step_pubILi%dELi512ELb1EEEvNS_7PubArgsE" % np_]
    assert int(tab["private_segment_fixed_size"]) == 0 and int(tab["vgpr_spill_count"]) == 0
    assert int(tab["vgpr_count"]) <= 256
    assert int(tab["group_segment_fixed_size"]) <= int(plain["group_segment_fixed_size"])


def test_codeobj_files_both_instances_under_one_name():
    from parakeet_slam_amd import codeobj

    h = codeobj.kernel_hashes()
    picked = [k for k in h if any(n in k for n in codeobj.KERNEL_SYMBOLS["k_step_pub<2, 512>"])]
    assert len(picked) == 2, picked
    assert any("k_colour_table" in k for k in h) and any("k_colour_rows" in k for k in h)

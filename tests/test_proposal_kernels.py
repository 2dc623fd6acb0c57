"""Host: the built library holds the measurement-informed proposal's kernels (k_propose, both instances of k_observe_proposed), and
their code-object metadata, read as test_kernel_resources.py reads it, says what DESIGN.md section 4 says: no scratch, nothing
spilled, 448 bytes of static LDS for k_propose's fourteen sums of four waves and block_sum's 32 for the observes, and for k_propose
three waves per SIMD (at most 168 VGPRs of 512)."""
import os

import pytest

from test_kernel_resources import READELF, code_object_kernels


def test_the_library_holds_the_proposal_kernels_without_scratch():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from parakeet_slam_amd import build

    ks = {k["symbol"]: k for k in code_object_kernels(build.build(verbose=False))}
    propose = [k for s, k in ks.items() if "9k_proposeE" in s]
    observed = [k for s, k in ks.items() if "k_observe_proposedILb" in s]
    assert len(propose) == 1 and len(observed) == 2, sorted(s for s in ks if "propose" in s)
    for k in propose + observed:
        assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == (14 * 4 * 8 if k in propose else 32), k  # fourteen sums x four waves; block_sum's
    assert int(propose[0]["vgpr_count"]) <= 168, propose[0]

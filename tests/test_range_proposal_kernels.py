"""Host: the built library holds the kernels of ranges in the proposal (k_propose_range, both instances of
k_observe_proposed_range) once each, and their code-object metadata, read as test_kernel_resources.py reads it, says what DESIGN.md
section 4 says: no scratch, nothing spilled to it, 480 bytes of static LDS for k_propose_range's fifteen sums of four waves and
block_sum's 32 for the observes.  VGPRs as found on this build (bounded by the 256 a 256-lane workgroup's wave can have):

    k_propose_range                      178   (two waves a SIMD; k_propose: 168, three)
    k_observe_proposed_range<true, 2>    188
    k_observe_proposed_range<false, 1>   177

k_propose itself is still one symbol, with at most 168 VGPRs."""
import os

import pytest

from test_kernel_resources import READELF, code_object_kernels


def test_the_library_holds_the_ranged_proposal_kernels_without_scratch():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from parakeet_slam_amd import build

    ks = {k["symbol"]: k for k in code_object_kernels(build.build(verbose=False))}
    propose = [k for s, k in ks.items() if "k_propose_rangeE" in s]
    known = [k for s, k in ks.items() if "k_observe_proposed_rangeILb1ELi2E" in s]
    ml = [k for s, k in ks.items() if "k_observe_proposed_rangeILb0ELi1E" in s]
    assert len(propose) == 1 and len(known) == 1 and len(ml) == 1, sorted(s for s in ks if "propose" in s)
    assert len([s for s in ks if "k_observe_proposed_rangeILb" in s]) == 2
    for k in propose + known + ml:
        assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == (15 * 4 * 8 if k in propose else 32), k  # fifteen sums x four waves; block_sum's
        assert int(k["vgpr_count"]) <= 256, k
    # ... and the kernels they stand beside are what they were
    plain = [k for s, k in ks.items() if "9k_proposeE" in s]
    assert len(plain) == 1 and int(plain[0]["vgpr_count"]) <= 168, plain
    assert int(plain[0]["group_segment_fixed_size"]) == 14 * 4 * 8
    assert len([s for s in ks if "k_observe_proposedILb" in s]) == 2

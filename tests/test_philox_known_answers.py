"""CPU: the NumPy restatement of pk_philox.hpp that the device-noise tests compare the GPU with (tests/test_gpu_parity.py) is
itself Philox4x32-10: Random123's published known answers (kat_vectors, philox4x32 10)."""
import numpy as np

from test_gpu_parity import device_normals, philox4x32_10

KNOWN = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_the_restatement_reproduces_the_published_known_answers():
    for counter, key, want in KNOWN:
        got = philox4x32_10(np.array([counter], dtype=np.uint32), key)
        assert [int(v) for v in got[0]] == list(want), (counter, key, ["%08x" % int(v) for v in got[0]])
    # rows are independent of each other
    got = philox4x32_10(np.array([KNOWN[2][0], KNOWN[0][0]], dtype=np.uint32), KNOWN[2][1])
    assert [int(v) for v in got[0]] == list(KNOWN[2][2])


def test_the_normals_read_all_four_counter_words():
    """device_normals: counter = (index low, index high, draw low, draw high | pair bit) -- no word is dropped on the way."""
    base = device_normals(8, 99, 3)
    assert np.all(np.isfinite(base)) and base.shape == (8, 3)
    assert np.array_equal(device_normals(4, 99, 3, offset=4), base[4:])
    for other in (device_normals(8, 99, 3, offset=2 ** 32), device_normals(8, 99, 3 + 2 ** 32), device_normals(8, 99 + 2 ** 32, 3)):
        assert not np.any(other == base)

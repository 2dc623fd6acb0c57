"""GPU: pk_device_bytes() is the device memory a filter holds NOW -- every block goes through one registry (csrc/pk_devmem.hpp,
DESIGN.md section 4 "Memory"), a regrow takes the old block's bytes out again, and pk_destroy gives everything back."""
import numpy as np
import pytest
import torch  # (before the library is loaded: the other way round torch finds no device)

from oracle.fastslam_oracle import synthetic_scan, synthetic_world

pytestmark = pytest.mark.gpu

POSE = (0.3, -0.2, 0.1)


def make_filter(lib, P, L, Qt=None, qt_first=False):
    means, covs = synthetic_world(L)
    f = lib.DeviceFilter(P, L)
    if Qt is not None and qt_first:
        f.set_measurement_noise(Qt)
    f.upload_map(means, covs.reshape(L, 25))
    if Qt is not None and not qt_first:
        f.set_measurement_noise(Qt)
    return f, means


def scan(means, n):
    """n blobs: blob j sees landmark j % L, repeated sightings a little off."""
    L = len(means)
    blobs = synthetic_scan(means, POSE)[np.arange(n) % L]
    blobs[:, 0] += 1e-3 * (np.arange(n) // L)
    return blobs


# what pk_device_bytes() returned right after pk_create in the commit before the registry (measured with that commit's library):
# nothing has been freed at that point, so the figure must not move
PARENT_BYTES_AFTER_CREATE = {(64, 8): 303984, (1000, 600): 141524224}


@pytest.mark.parametrize("P,L", sorted(PARENT_BYTES_AFTER_CREATE))
def test_bytes_after_create_unchanged(lib, P, L):
    f = lib.DeviceFilter(P, L)
    got = f.device_bytes()
    f.close()
    print("device_bytes after create, P=%d L=%d: %d" % (P, L, got))
    assert got == PARENT_BYTES_AFTER_CREATE[(P, L)]


@pytest.mark.parametrize("L,known_ids", [(600, False), (8, True)])
def test_bytes_do_not_depend_on_history(lib, L, known_ids):
    """Scans of 2, 40 and 300 blobs against the 300-blob scan alone.  Every buffer's capacity is a function of the need that last
    made it grow, and the 300-blob scan outgrows what the 40-blob one left (the widest slack is 40 + 40 / 4 + 64 = 114 < 300), so
    both filters end with the same blocks.  (Before the registry the first one also counted the blocks it had freed.)"""
    P = 256
    got = []
    for sizes in ((2, 40, 300), (300,)):
        f, means = make_filter(lib, P, L)
        for n in sizes:
            blobs = scan(means, n)
            f.observe(blobs, ids=(np.arange(n) % L + 1).astype(np.int32) if known_ids else None)
        f.resample(0.37)
        f.synchronize()
        got.append(f.device_bytes())
        f.close()
    print("device_bytes, L=%d: after 2 / 40 / 300 blobs %d, after 300 blobs alone %d" % (L, got[0], got[1]))
    assert got[0] == got[1]


def test_bytes_after_the_switch_to_the_dense_layout(lib):
    """A coupled Qt moves the maps to the dense layout: the compact maps' bytes leave the figure with them."""
    P, L = 64, 40
    Qt = 0.1 * np.identity(4)
    Qt[0, 1] = Qt[1, 0] = 0.02  # bearing-colour coupling
    got = []
    for qt_first in (False, True):  # the map goes in compact and is converted | the filter is dense before its map arrives
        f, means = make_filter(lib, P, L, Qt, qt_first)
        f.observe(scan(means, 12))
        assert f.observe_route() == "dense"
        got.append(f.device_bytes())
        f.close()
    print("device_bytes on the dense layout: switched %d, dense from the start %d" % tuple(got))
    assert got[0] == got[1]


# hipMemGetInfo moves in steps of this many bytes (seen on the MI355X: of 4 096 hipMalloc calls of one byte each every 512th lowers
# the free figure by 2 MiB and the others by nothing; one block of 4 KiB, 64 KiB or 1 MiB lowers it by 2 MiB, one of 2 MiB + 1 by 4 MiB)
ALLOC_GRANULE = 2 << 20
# free memory at the end of cycle 1 minus free memory at the end of cycle 20 in the test below, with the library of the commit before
# the registry (pk_destroy freed from hand-kept lists of buffers): 0 bytes.  With the registry, when this was written: 0 bytes too.
PARENT_DROP_OVER_20_CYCLES = 0


def test_destroy_returns_the_memory(lib):
    """create (4096 x 600), three growing observes, close -- twenty times in one process.  Nothing may stay behind that the old
    pk_destroy, which named every buffer, gave back: the free memory after cycle 20 is that after cycle 1, to within the drop the
    old library showed plus one allocation granule."""
    free_after = []
    for cycle in range(20):
        f, means = make_filter(lib, 4096, 600)
        for n in (2, 40, 300):
            f.observe(scan(means, n))
        f.synchronize()
        f.close()
        free_after.append(torch.cuda.mem_get_info()[0])
    drop = free_after[0] - free_after[-1]
    print("free memory after cycle 1 minus after cycle 20: %d bytes (free after each cycle: %s)" % (drop, free_after))
    assert drop <= PARENT_DROP_OVER_20_CYCLES + ALLOC_GRANULE
